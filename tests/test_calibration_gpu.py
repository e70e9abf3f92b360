"""``dct_calibration_counts`` / ``CalibrationMeter`` / the calibration and reliability tables of ``summary.summarize`` / ``CoTrainer``'s
``val_calibration`` on the GPU, against the numpy reference of test_calibration_cpu.py.

Probabilities in, S a power of two: every step that decides an integer is reproducible in fp32 (the ensemble mean is a sum and an exact
scaling, the bin one multiply, the confidence word an exact scaling and a truncation), so ``bins`` is compared with ``np.array_equal``.
``scores`` (Brier, NLL) holds truncated fp32 sums of squares and logf: compared as means against the float64 reference computed from the
same fp32 probabilities.  Tolerance rule: four times the largest deviation observed over the cases of this file, never above 1e-4.
Observed on an MI355X: Brier 1.556e-8, NLL 2.410e-6 (SCORE_OBSERVED); chosen: 6.2e-8 and 9.6e-6 (SCORE_TOL).  The Brier figure is the
truncation to 2^-24 = 6e-8 steps; the NLL figure is one fp32 rounding of logf near 23, the same on every wrong pixel of a one-hot map.

Logits in (fp32 softmax on the device, float64 in the reference), or S = 3 (a division by 3): a pixel within 1e-4 of a bin edge, or whose
top two probabilities differ by less than 1e-5, may land in a neighbouring bin or lose its tie-break.  Those "uncertain" pixels (at most
0.2 % of the pixels, asserted) bound every count cell from both sides; the totals are exact; ECE, Brier and NLL are measured the same
way (observed ECE 3.100e-8, Brier 1.408e-8, NLL 1.565e-7: LOGITS_OBSERVED; chosen four times that: LOGITS_TOL), ECE capped by twice
the uncertain share of the case as well."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FakeLoader, batches  # noqa: E402
from test_calibration_cpu import UNIT, derived, noise_probs, reference  # noqa: E402

DEV = "cuda:0"
CAP = 1e-4
# largest |mean Brier - ref|, |mean NLL - ref| observed over the exact cases / |ECE - ref|, Brier, NLL over the logits cases
SCORE_OBSERVED = {"Brier": 1.556e-8, "NLL": 2.410e-6}          # Brier: C = 2 noise; NLL: one-hot maps, logf(1e-10f) on every wrong pixel
SCORE_TOL = {k: min(CAP, 4 * v) for k, v in SCORE_OBSERVED.items()}                 # 6.2e-8, 9.6e-6
LOGITS_OBSERVED = {"ECE": 3.100e-8, "Brier": 1.408e-8, "NLL": 1.565e-7}
LOGITS_TOL = {k: min(CAP, 4 * v) for k, v in LOGITS_OBSERVED.items()}               # 1.2e-7, 5.6e-8, 6.3e-7


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def run(views, gt, n_bins, classes=None, ens=True, logits=False):
    from dct_amd import hip_ops as K
    bins, scores = K.calibration_counts([dev(v, np.float32) for v in views], dev(gt, np.int64), n_bins=n_bins, classes=classes,
                                        with_ensemble=ens, from_logits=logits)
    B, R = views[0].shape[0], len(views) + int(ens)
    assert bins.dtype == torch.int64 and tuple(bins.shape) == (B, R, n_bins, 3)
    assert scores.dtype == torch.int64 and tuple(scores.shape) == (B, R, 2)
    return bins.cpu().numpy(), scores.cpu().numpy()


def flat(views):
    return [v.reshape(v.shape[0], -1, v.shape[-1]) for v in views]


def check_scores(got_bins, got_scores, ref, tol, what):
    _, _, brier, nll = derived(got_bins, got_scores[..., 0] / UNIT, got_scores[..., 1] / UNIT)
    _, _, rbrier, rnll = derived(ref["bins"], ref["brier"], ref["nll"])
    assert np.array_equal(np.isnan(brier), np.isnan(rbrier))
    devs = {"Brier": float(np.nanmax(np.abs(brier - rbrier), initial=0.0)), "NLL": float(np.nanmax(np.abs(nll - rnll), initial=0.0))}
    print(f"DEV {what} Brier {devs['Brier']:.3e} NLL {devs['NLL']:.3e}")
    for k, d in devs.items():
        assert d <= tol[k], (what, k, d)


def check_exact(views, gt, n_bins, classes=None, ens=True, what=""):
    ref = reference(flat(views), gt, n_bins, classes=classes, with_ensemble=ens, exact=True)
    bins, scores = run(views, gt, n_bins, classes=classes, ens=ens)
    print(what, "non-zero cells", int((ref["bins"] != 0).sum()), "of", ref["bins"].size, "counted", int(ref["N"].sum()))
    assert np.array_equal(bins, ref["bins"]), (what, np.argwhere(bins != ref["bins"])[:10])
    check_scores(bins, scores, ref, SCORE_TOL, what)
    return bins, scores, ref


def noise_case(seed, B, H, W, C, S, sharp=2.0):
    rng = np.random.default_rng(seed)
    return [noise_probs(rng, B, H * W, C, sharp).reshape(B, H, W, C) for _ in range(S)], rng.integers(0, C, (B, H, W))


# ---------------------------------------------------------------------------------------------------------------- exact tables
@pytest.mark.parametrize("B,H,W,C,S", [(1, 1, 1, 2, 1), (2, 5, 7, 4, 2), (3, 37, 53, 3, 2), (3, 37, 53, 4, 4), (1, 130, 130, 4, 2),
                                       (2, 37, 53, 4, 1)])
def test_shapes(B, H, W, C, S):
    """1x1: one lane; 5x7: an image smaller than a wave; 37x53: a partial last wave, odd strides; 130x130 = 16900 pixels: more than
    one pass of the grid (64 blocks of 256), so the grid-stride loop runs."""
    views, gt = noise_case(B * 1000 + W + S, B, H, W, C, S)
    bins, _, _ = check_exact(views, gt, 15, what=f"noise {B}x{H}x{W}x{C} S={S}")
    assert (bins[..., 0].sum(-1) == H * W).all()
    if S == 1:
        assert np.array_equal(bins[:, 0], bins[:, 1])           # the mean of one view is that view
    alone, _ = run(views, gt, 15, ens=False)
    assert np.array_equal(alone, bins[:, :S])


@pytest.mark.parametrize("C", [2, 3, 4, 5, 8])
def test_class_counts(C):
    """The vector loads (C = 4, C = 2) and the scalar ones."""
    views, gt = noise_case(70 + C, 2, 19, 23, C, 2, sharp=3.0)
    check_exact(views, gt, 10, what=f"C={C}")


def test_full_table_four_views_32_bins_8_classes():
    rng = np.random.default_rng(11)
    B, P, C, S = 2, 64 * 64, 8, 4
    sharp = rng.uniform(0.2, 6.0, (B, P, 1))                    # from flat to peaked: confidences from 1/8 to 1
    views = []
    for _ in range(S):
        x = rng.normal(0, 1, (B, P, C)) * sharp
        e = np.exp(x - x.max(-1, keepdims=True))
        views.append((e / e.sum(-1, keepdims=True)).astype(np.float32).reshape(B, 64, 64, C))
    gt = rng.integers(0, C, (B, 64, 64))
    bins, _, ref = check_exact(views, gt, 32, what="full table")
    assert (ref["bins"][:, :, 4:, 0] > 0).mean() > 0.9          # (bins below 1/8 cannot be reached at C = 8)


def test_every_pixel_in_one_bin():
    B, H, W = 2, 9, 11
    gt = np.random.default_rng(3).integers(0, 4, (B, H, W))
    quarter = np.full((B, H, W, 4), 0.25, dtype=np.float32)     # conf * n_bins is exactly 1.0: bin 1; every tie goes to class 0
    bins, scores, _ = check_exact([quarter, quarter], gt, 4, what="all 0.25")
    for b in range(B):
        assert bins[b, :, 1].tolist() == [[H * W, int((gt[b] == 0).sum()), H * W * (1 << 22)]] * 3
    assert int(bins[:, :, [0, 2, 3]].sum()) == 0
    onehot = np.eye(4, dtype=np.float32)[np.random.default_rng(4).integers(0, 4, (B, H, W))]
    bins, _, _ = check_exact([onehot, onehot], gt, 4, what="one-hot")       # conf = 1.0: the last bin, not one past it
    assert (bins[:, :, 3, 0] == H * W).all() and (bins[:, :, 3, 2] == H * W * (1 << 24)).all() and int(bins[:, :, :3].sum()) == 0
    bins, _, _ = check_exact([onehot], gt, 32, ens=False, what="one-hot, 32 bins")
    assert (bins[:, :, 31, 0] == H * W).all()


def test_exact_ties_go_to_the_first_class():
    p = np.array([[0.4, 0.4, 0.2], [0.2, 0.4, 0.4], [0.25, 0.5, 0.25], [1 / 3, 1 / 3, 1 / 3]], dtype=np.float32)
    views = [np.tile(p, (1, 3, 1)).reshape(1, 1, 12, 3)]        # every pattern against every gt
    gt = np.repeat(np.arange(3), 4).reshape(1, 1, 12)
    bins, _, ref = check_exact(views, gt, 10, ens=False, what="ties")
    # right: (0.4, 0.4, 0.2) with gt 0, (0.2, 0.4, 0.4) with gt 1, (0.25, 0.5, 0.25) with gt 1, thirds with gt 0
    assert int(bins[..., 1].sum()) == 4 and bins[0, 0, 4, :2].tolist() == [6, 2] and bins[0, 0, 3, :2].tolist() == [3, 1]


def test_invalid_gt_is_skipped_and_the_class_mask_equals_masking_the_pixels():
    views, gt = noise_case(21, 3, 37, 53, 4, 2)
    gt[0, :3, :] = 255
    gt[1, 5, :] = -1
    gt[2, :, 7] = 4                                             # = C
    bins, _, ref = check_exact(views, gt, 15, what="invalid gt")
    assert bins[..., 0].sum(-1)[:, 0].tolist() == [37 * 53 - 3 * 53, 37 * 53 - 53, 37 * 53 - 37]
    masked, mscores, _ = check_exact(views, gt, 15, classes=[1, 3], what="class mask")
    dropped = np.where((gt == 1) | (gt == 3), gt, 255)
    plain, pscores = run(views, dropped, 15)
    assert np.array_equal(masked, plain) and np.array_equal(mscores, pscores)
    assert np.array_equal(masked, reference(flat(views), dropped, 15, with_ensemble=True)["bins"])


def test_all_gt_invalid_gives_empty_tables_and_nan():
    from dct_amd.metrics import CalibrationMeter, ece_of
    views, gt = noise_case(22, 2, 20, 20, 3, 2)
    bins, scores = run(views, np.full_like(gt, 255), 15)
    assert not bins.any() and not scores.any() and np.isnan(ece_of(bins)).all()
    bins, scores = run(views, np.zeros_like(gt), 15, classes=[1, 2])
    assert not bins.any() and not scores.any()
    m = CalibrationMeter(method='2d', C=3, n_models=2, considered_classes=[1, 2])
    m.add([dev(v, np.float32).permute(0, 3, 1, 2) for v in views], dev(np.zeros_like(gt), np.int64).unsqueeze(1))
    for got in (m.ece(), m.mce(), m.brier(), m.nll()):
        assert np.isnan(got[0].numpy()).all() and got[2].tolist() == [0, 0, 0]
    assert np.isnan(m.summary()["mECE"]) and int(m.tables().sum()) == 0


def test_two_calls_are_bit_identical_and_the_call_adds():
    from dct_amd import _lib, hip_ops as K
    views, gt = noise_case(23, 2, 64, 64, 4, 4)
    ps, g = [dev(v, np.float32) for v in views], dev(gt, np.int64)
    a = K.calibration_counts(ps, g, n_bins=32, with_ensemble=True)
    b = K.calibration_counts(ps, g, n_bins=32, with_ensemble=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    bins, scores = a[0].clone(), a[1].clone()                   # holds earlier sums: the call adds
    _lib.call("dct_calibration_counts", K._ptr_array(ps), 4, g.data_ptr(), 2, 64 * 64, 4, 32, 15, 1, 0, bins.data_ptr(), scores.data_ptr(),
              _lib.stream())
    assert torch.equal(bins, 2 * a[0]) and torch.equal(scores, 2 * a[1])


def test_views_of_any_layout_get_dense_copies():
    from dct_amd import hip_ops as K
    views, gt = noise_case(24, 3, 12, 10, 4, 2)
    ref = reference(flat(views), gt, 15, with_ensemble=True)["bins"]
    ps, g = [dev(v, np.float32) for v in views], dev(gt, np.int64)
    assert np.array_equal(K.calibration_counts([p[1:] for p in ps], g[1:], with_ensemble=True)[0].cpu().numpy(), ref[1:])
    nchw = [p.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1) for p in ps]
    assert np.array_equal(K.calibration_counts(nchw, g.to(torch.int32), with_ensemble=True)[0].cpu().numpy(), ref)
    assert np.array_equal(K.calibration_counts([p.double() for p in ps], g.reshape(3, -1), with_ensemble=True)[0].cpu().numpy(), ref)


# ----------------------------------------------------------------------------------------------------- logits, S = 3 and S = 8
@pytest.mark.parametrize("C,S,n_bins,scale", [(4, 2, 15, 2.0), (4, 3, 15, 1.0), (2, 2, 10, 3.0), (8, 8, 32, 2.0), (3, 3, 15, 3.0)])
def test_from_logits_within_the_uncertain_pixels(C, S, n_bins, scale):
    rng = np.random.default_rng(100 * C + S)
    B, H, W = 2, 64, 64
    views = [(rng.normal(0, scale, (B, H, W, C))).astype(np.float32) for _ in range(S)]
    gt = rng.integers(0, C, (B, H, W))
    gt[0, 0, :9] = 255
    ref = reference(flat(views), gt, n_bins, with_ensemble=True, from_logits=True, exact=False)
    share = float(ref["uncertain"].mean())
    print(f"logits C={C} S={S} n_bins={n_bins}: uncertain share {share:.5f}")
    assert share <= 0.002
    bins, scores = run(views, gt, n_bins, logits=True)
    assert np.array_equal(bins[..., 0].sum(-1), np.broadcast_to(ref["N"][:, None], (B, S + 1)))          # totals per image and rater
    for r in range(S + 1):
        for b in range(B):
            m = ref["counted"][b]
            unc = m & ref["uncertain"][r, b]
            cert = m & ~ref["uncertain"][r, b]
            k = ref["bin"][r, b]
            at = np.bincount(k[unc], minlength=n_bins)
            room = at + np.append(at[1:], 0) + np.append(0, at[:-1])       # an uncertain pixel lands in its bin or a neighbour
            for col, sel in ((0, cert), (1, cert & ref["correct"][r, b])):
                lo = np.bincount(k[sel], minlength=n_bins)
                got = bins[b, r, :, col]
                assert (lo <= got).all() and (got <= lo + room).all(), (r, b, col, lo, got, room)
    ece, _, brier, nll = derived(bins, scores[..., 0] / UNIT, scores[..., 1] / UNIT)
    rece, _, rbrier, rnll = derived(ref["bins"], ref["brier"], ref["nll"])
    devs = {"ECE": float(np.abs(ece - rece).max()), "Brier": float(np.abs(brier - rbrier).max()), "NLL": float(np.abs(nll - rnll).max())}
    print(f"LOGITSDEV C={C} S={S} ECE {devs['ECE']:.3e} Brier {devs['Brier']:.3e} NLL {devs['NLL']:.3e} (ECE cap {2 * share:.3e})")
    assert devs["ECE"] <= min(LOGITS_TOL["ECE"], 2 * share) and devs["Brier"] <= LOGITS_TOL["Brier"] and devs["NLL"] <= LOGITS_TOL["NLL"]


# ------------------------------------------------------------------------------------------------------------ through the layers
@pytest.mark.parametrize("method", ["2d", "3d"])
def test_meter_row_by_row(method):
    from dct_amd.metrics import CalibrationMeter
    C, S, nb, classes = 4, 2, 15, [1, 2, 3]
    m = CalibrationMeter(method=method, C=C, n_models=S, with_ensemble=True, n_bins=nb, considered_classes=classes)
    rows_bins, rows_brier, rows_nll = [], [], []
    for i in range(3):
        views, gt = noise_case(300 + i, 3, 24, 20, C, S, sharp=1.0 + i)
        if i == 1:
            gt[0] = 0                                           # a slice without a counted pixel
        m.add([dev(v, np.float32).permute(0, 3, 1, 2) for v in views], dev(gt, np.int64).unsqueeze(1))
        ref = reference(flat(views), gt, nb, classes=classes, with_ensemble=True)
        if method == "3d":
            rows_bins.append(ref["bins"].sum(0, keepdims=True)); rows_brier.append(ref["brier"].sum(0, keepdims=True))
            rows_nll.append(ref["nll"].sum(0, keepdims=True))
        else:
            rows_bins.append(ref["bins"]); rows_brier.append(ref["brier"]); rows_nll.append(ref["nll"])
    rb, rbr, rnl = np.concatenate(rows_bins), np.concatenate(rows_brier), np.concatenate(rows_nll)
    assert np.array_equal(m._rows()[0], rb) and np.array_equal(m.tables().numpy(), rb.sum(0))
    check_scores(*m._rows(), dict(bins=rb, brier=rbr, nll=rnl), SCORE_TOL, f"meter {method}")          # row by row
    ece, mce, brier, nll = derived(rb, rbr, rnl)
    n_rows = 3 if method == "3d" else 9
    assert ece.shape == (n_rows, 3) and int(np.isnan(ece[:, 0]).sum()) == (0 if method == "3d" else 1)
    for got, want, tol in ((m.ece(), ece, 1e-12), (m.mce(), mce, 1e-12), (m.brier(), brier, SCORE_TOL["Brier"]), (m.nll(), nll, SCORE_TOL["NLL"])):
        mean, std, defined = (x.numpy() for x in got)
        assert defined.tolist() == [int((~np.isnan(want[:, r])).sum()) for r in range(3)]
        # rows within tol of the reference: so is their mean, and their std within sqrt(n / (n - 1)) tol <= 2 tol
        assert np.allclose(mean, np.nanmean(want, 0), rtol=0, atol=tol) and np.allclose(std, np.nanstd(want, 0, ddof=1), rtol=0, atol=2 * tol)
    assert list(m.detailed_summary()) == ["S0", "S1", "ensemble"]


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b or (a != a and b != b)


def _segmentators(C, n=2):
    from dct_amd.models import Segmentator
    segs = []
    for seed in range(n):
        torch.manual_seed(40 + seed)
        segs.append(Segmentator({"name": "enet", "num_classes": C, "compute_dtype": torch.float32}, {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4},
                                {"name": "StepLR", "step_size": 90, "gamma": 0.1}))
    return segs


def test_summarize_calibration_and_reliability_tables():
    from dct_amd import summary
    from dct_amd.metrics import CalibrationMeter
    C, H, nb = 3, 32, 10
    models = _segmentators(C)
    val = FakeLoader(batches(91, 4, 1, H, C), 1)
    plain = summary.summarize(models, val, DEV, "soft", report_axises=[1, 2], kappa=True)
    res = summary.summarize(models, val, DEV, "soft", report_axises=[1, 2], kappa=True, calibration=True, calibration_bins=nb,
                            calibration_classes=[1, 2])
    assert sorted(res) == sorted(list(plain) + ["calibration_2d", "calibration_3d", "reliability"])
    assert _same({k: res[k] for k in plain}, plain)
    hard = summary.summarize(models, val, DEV, "hard", report_axises=[1, 2], largest_component="2d", calibration=True, calibration_bins=nb,
                             calibration_classes=[1, 2])
    assert not [k for k in hard if k.endswith("_lcc") and ("calibration" in k or "reliability" in k)]
    assert all(_same(hard[k], res[k]) for k in ("calibration_2d", "calibration_3d", "reliability"))      # always the mean of the probabilities
    keys = ["model_0", "model_1", "ensemble"]
    for method in ("2d", "3d"):
        meter = CalibrationMeter(method=method, C=C, n_models=2, with_ensemble=True, n_bins=nb, considered_classes=[1, 2])
        with torch.no_grad():
            for (img, gt), _, _ in val:
                meter.add([m.predict(img.to(DEV), logit=False) for m in models], gt.to(DEV))
        t = res["calibration_" + method]
        assert list(t) == keys + ["ensemble_std"]
        stats = {"ECE": meter.ece(), "MCE": meter.mce(), "Brier": meter.brier(), "NLL": meter.nll()}
        for r, key in enumerate(keys):
            assert _same(t[key], {k: float(v[0][r]) for k, v in stats.items()})
        assert _same(t["ensemble_std"], {k: float(v[1][2]) for k, v in stats.items()})
        assert all(0 <= t[key]["ECE"] <= t[key]["MCE"] <= 1 for key in keys)
    count, acc, conf = meter.reliability()
    cov, kept = meter.coverage_accuracy()
    t = res["reliability"]
    assert list(t) == keys
    for r, key in enumerate(keys):
        assert _same(t[key], {"count": count[r].tolist(), "accuracy": acc[r].tolist(), "confidence": conf[r].tolist(),
                              "coverage": cov[r].tolist(), "kept_accuracy": kept[r].tolist()})
        assert len(t[key]["count"]) == nb and t[key]["coverage"][0] == 1.0
    print(res["calibration_3d"], res["reliability"]["ensemble"])


class _Recorder(object):
    def __init__(self):
        self.calls = []

    def add_scalars(self, tag, values, epoch):
        self.calls.append((tag, dict(values), epoch))


def test_eval_loop_uploads_val_calibration_only_on_request(tmp_path):
    from dct_amd import ModelMode
    from dct_amd.loss import get_loss_fn
    from dct_amd.metrics import CalibrationMeter
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
    withc = CoTrainer(segs, lab, val, val, crit, save_dir=str(tmp_path / "b"), val_calibration=True, **kw)
    plain.writer, withc.writer = _Recorder(), _Recorder()
    with torch.no_grad():
        a2, a3 = plain._eval_loop(val, epoch=0, mode=ModelMode.EVAL, save=False)
        b2, b3 = withc._eval_loop(val, epoch=0, mode=ModelMode.EVAL, save=False)
    assert torch.equal(a2, b2) and torch.equal(a3, b3)
    assert not [c for c in plain.writer.calls if c[0].startswith("val_calibration")]
    assert [c for c in plain.writer.calls if c[0].startswith("val_data")] == [c for c in withc.writer.calls if c[0].startswith("val_data")]
    assert [c[0] for c in plain.writer.calls] == [c[0] for c in withc.writer.calls if not c[0].startswith("val_calibration")]
    cal = {c[0]: c[1] for c in withc.writer.calls if c[0].startswith("val_calibration/")}
    assert sorted(cal) == ["val_calibration/S0", "val_calibration/S1", "val_calibration/ensemble"]
    meter = CalibrationMeter(method="3d", C=C, n_models=2, with_ensemble=True, considered_classes=[1, 2], from_logits=True)
    with torch.no_grad():
        for (img, gt), _, _ in val:
            meter.add([seg.predict(img.to(DEV), logit=True) for seg in segs], gt.to(DEV))
    d = meter.detailed_summary()
    for name in ("S0", "S1", "ensemble"):
        assert list(cal[f"val_calibration/{name}"]) == ["ECE", "NLL", "Brier"]
        assert _same(cal[f"val_calibration/{name}"], {k: d[name][k] for k in ("ECE", "NLL", "Brier")})
        assert 0 <= d[name]["ECE"] <= 1 and d[name]["NLL"] > 0
    print(cal)


def test_calibrated_probabilities_beat_their_sharpened_copy():
    """gt sampled from the probabilities themselves: those are calibrated by construction (ECE ~ the sampling noise); the same logits
    at a temperature of 0.5 are over-confident.  One launch, the two as views 0 and 1."""
    from dct_amd.metrics import CalibrationMeter
    rng = np.random.default_rng(8)
    B, H, W, C = 8, 64, 64, 4
    x = rng.normal(0, 1.5, (B, H, W, C)).astype(np.float32)
    p = np.exp(x.astype(np.float64) - x.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    gt = (rng.random((B, H, W, 1)) > p.cumsum(-1)).sum(-1).clip(0, C - 1)
    m = CalibrationMeter(method='3d', C=C, n_models=2, with_ensemble=False, n_bins=15, from_logits=True, rater_names=["T1", "T0.5"])
    m.add([dev(x, np.float32).permute(0, 3, 1, 2), dev(2 * x, np.float32).permute(0, 3, 1, 2)], dev(gt, np.int64).unsqueeze(1))
    d = m.detailed_summary()
    print(d)
    assert d["T1"]["ECE"] < 0.02 < 0.05 < d["T0.5"]["ECE"]
    assert d["T1"]["NLL"] < d["T0.5"]["NLL"] and d["T1"]["Brier"] < d["T0.5"]["Brier"]
    cov, kept = m.coverage_accuracy()
    assert float(cov[0, 0]) == 1.0 and (np.diff(kept[0].numpy()[~np.isnan(kept[0].numpy())]) > -0.02).all()      # more confident, more right
