"""``dct_temperature_sums`` / ``dct_temperature_apply`` / ``metrics.TemperatureScaler`` / the temperature tables of ``summary.summarize``
on the GPU, against the numpy reference of temperature_ref.py.

The sums are compared as means over the counted pixels (mean NLL, mean d NLL / d beta) with the float64 reference computed from the same
fp32 logits and the same fp32 candidates; ``counted`` is exact.  Tolerance rule: four times the largest deviation observed over the cases
of this file, never above 1e-4.  Observed on an MI355X: NLL 1.176e-6, G 5.089e-7 (SUMS_OBSERVED; both on the single-pixel case, where one
word's rounding to 2^-20 is not averaged away); chosen four times that: 4.7e-6 and 2.0e-6 (SUMS_TOL).  The fitted inverse temperature is compared with the fit of the same solver on the float64 reference in
|ln beta - ln beta_ref|: observed 4.881e-8 (FIT_OBSERVED), chosen four times that, 2.0e-7, never above 1e-3 (FIT_TOL).

Exact on the device: two runs, the added call, the class mask against dropped pixels, the words of (2 z, beta / 2) against (z, beta), and
the calibration tables of the probabilities applied at beta = 1 against those the calibration kernel forms from the logits.

The applied probabilities against float64: |p - ref| <= 1e-5 (APPLY_TOL), from the formats: with |beta z| <= 32 the rounded product and
its distance to the maximum are each off by at most 2^-24 * 32 = 1.9e-6, expf and the division add a few 2^-24, so a probability
(<= 1) is off by less than 5e-6 relative; the ensemble's logits inherit that from the views' softmax at |z| <= 8 (1e-6) times beta <= 2.
Observed on an MI355X: 2.8e-7 at most."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FakeLoader, batches  # noqa: E402
from temperature_ref import UNIT, applied, reference, sampled_case, sum_fn_of  # noqa: E402

DEV = "cuda:0"
CAP, FIT_CAP = 1e-4, 1e-3
SUMS_OBSERVED = {"NLL": 1.176e-6, "G": 5.089e-7}          # both on the one-pixel case; above 1000 pixels: 5.8e-7, 1.3e-7
SUMS_TOL = {k: min(CAP, 4 * v) for k, v in SUMS_OBSERVED.items()}                   # 4.7e-6, 2.0e-6
FIT_OBSERVED = 4.881e-8
FIT_TOL = min(FIT_CAP, 4 * FIT_OBSERVED)                    # 2.0e-7
APPLY_TOL = 1e-5


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def flat(views):
    return [v.reshape(v.shape[0], -1, v.shape[-1]) for v in views]


def noise_case(seed, B, H, W, C, S, scale=2.0):
    rng = np.random.default_rng(seed)
    return [rng.normal(0, scale, (B, H, W, C)).astype(np.float32) for _ in range(S)], rng.integers(0, C, (B, H, W))


def candidates(R, K, span=3.0):
    """[R, K] fp32 inverse temperatures between 2^-span and 2^span, another grid for every rater."""
    return np.stack([np.exp2(np.linspace(-span, span, K) + 0.1 * r) for r in range(R)]).astype(np.float32)


def run(views, gt, betas, classes=None, ens=True, out=None):
    from dct_amd import hip_ops as K
    sums, counted = K.temperature_sums([dev(v, np.float32) for v in views], dev(gt, np.int64), dev(betas, np.float32), classes=classes,
                                       with_ensemble=ens, out=out)
    R = len(views) + int(ens)
    assert sums.dtype == torch.int64 and tuple(sums.shape) == (R, betas.shape[1], 2)
    assert counted.dtype == torch.int64 and counted.numel() == 1
    return sums.cpu().numpy(), int(counted.cpu())


def check(views, gt, betas, classes=None, ens=True, what=""):
    ref = reference(flat(views), gt, betas.astype(np.float64), classes=classes, with_ensemble=ens)
    sums, counted = run(views, gt, betas, classes=classes, ens=ens)
    assert counted == ref["N"], (what, counted, ref["N"])
    if counted == 0:
        assert not sums.any()
        return sums, counted
    devs = {"NLL": float(np.abs(sums[..., 0] / (UNIT * counted) - ref["nll"] / counted).max()),
            "G": float(np.abs(sums[..., 1] / (UNIT * counted) - ref["g"] / counted).max())}
    print(f"DEV {what} counted {counted} NLL {devs['NLL']:.3e} G {devs['G']:.3e}")
    for k, d in devs.items():
        assert d <= SUMS_TOL[k], (what, k, d)
    return sums, counted


# ------------------------------------------------------------------------------------------------------------------- the sums
@pytest.mark.parametrize("B,H,W,C,S", [(1, 1, 1, 2, 1), (2, 5, 7, 4, 2), (3, 37, 53, 3, 2), (1, 130, 130, 4, 2)])
def test_shapes(B, H, W, C, S):
    """1x1: one lane; 5x7: an image smaller than a wave; 37x53: a partial last wave, scalar loads; 130x130 = 16900 pixels: more than
    one pass of the grid (64 blocks of 256), so the grid-stride loop runs.  16 candidates: four chunks."""
    views, gt = noise_case(B * 1000 + W + S, B, H, W, C, S)
    betas = candidates(S + 1, 16)
    sums, counted = check(views, gt, betas, what=f"noise {B}x{H}x{W}x{C} S={S}")
    assert counted == B * H * W
    alone, n = run(views, gt, betas[:S], ens=False)
    assert n == counted and np.array_equal(alone, sums[:S])
    if counted >= 1000:                                         # (a handful of pixels: the last word of a lane may wobble)
        assert (np.diff(sums[..., 1], axis=1) >= 0).all()       # the gradient sum is non-decreasing in beta


@pytest.mark.parametrize("C", [2, 3, 4, 5, 8])
def test_class_counts(C):
    """The vector loads (C = 4, C = 2) and the scalar ones; 5 candidates: a whole chunk and a partial one."""
    views, gt = noise_case(70 + C, 2, 19, 23, C, 2, scale=3.0)
    check(views, gt, candidates(3, 5), what=f"C={C}")


@pytest.mark.parametrize("S,C,K,H,W", [(8, 8, 16, 24, 20), (3, 4, 7, 31, 17), (4, 2, 16, 31, 17), (5, 3, 3, 31, 17), (1, 4, 1, 31, 17)])
def test_view_counts_and_candidate_counts(S, C, K, H, W):
    """S = 8, C = 8, K = 16: the largest instantiation (chunks of two candidates from five views on); S = 3, 4: the four-view form;
    K = 7, 3: partial chunks; K = 1."""
    views, gt = noise_case(200 + S, 2, H, W, C, S)
    check(views, gt, candidates(S + 1, K, span=2.0), what=f"S={S} C={C} K={K}")


def test_invalid_gt_is_skipped_and_the_class_mask_equals_masking_the_pixels():
    views, gt = noise_case(21, 3, 37, 53, 4, 2)
    gt[0, :3, :] = 255
    gt[1, 5, :] = -1
    gt[2, :, 7] = 4                                             # = C
    betas = candidates(3, 6)
    _, counted = check(views, gt, betas, what="invalid gt")
    assert counted == 3 * 37 * 53 - 3 * 53 - 53 - 37
    masked, n = check(views, gt, betas, classes=[1, 3], what="class mask")
    plain, m = run(views, np.where((gt == 1) | (gt == 3), gt, 255), betas)
    assert n == m and np.array_equal(masked, plain)


def test_nothing_counted_gives_zero_sums_and_a_nan_fit():
    from dct_amd.metrics import TemperatureScaler
    views, gt = noise_case(22, 2, 20, 20, 3, 2)
    check(views, np.full_like(gt, 255), candidates(3, 4), what="all invalid")
    check(views, np.zeros_like(gt), candidates(3, 4), classes=[1, 2], what="all masked")
    s = TemperatureScaler(C=3, n_models=2, considered_classes=[1, 2])
    s.fit([([dev(v, np.float32).permute(0, 3, 1, 2) for v in views], dev(np.zeros_like(gt), np.int64).unsqueeze(1))])
    assert np.isnan(s.temperature.numpy()).all() and np.isnan(s.nll_after.numpy()).all() and s.at_bound == [None] * 3
    assert np.isnan(s.detailed_summary()["ensemble"]["T"])


def test_two_calls_are_bit_identical_and_the_call_adds():
    views, gt = noise_case(23, 2, 64, 64, 4, 4)
    betas = candidates(5, 16)
    a, n = run(views, gt, betas)
    b, m = run(views, gt, betas)
    assert n == m and np.array_equal(a, b)
    from dct_amd import hip_ops as K
    zs, g, bt = [dev(v, np.float32) for v in views], dev(gt, np.int64), dev(betas, np.float32)
    first = K.temperature_sums(zs, g, bt, with_ensemble=True)
    again = K.temperature_sums(zs, g, bt, with_ensemble=True, out=first)
    assert again[0] is first[0] and np.array_equal(first[0].cpu().numpy(), 2 * a) and int(first[1].cpu()) == 2 * n


def test_doubled_logits_at_half_beta_give_the_same_nll_words():
    """x = beta z is the same fp32 number, so every NLL word is the same; g doubles exactly and each word is rounded once."""
    views, gt = noise_case(24, 2, 37, 53, 4, 2)
    betas = candidates(2, 16)
    a, n = run(views, gt, betas, ens=False)
    b, _ = run([2 * v for v in views], gt, betas / 2, ens=False)
    assert np.array_equal(a[..., 0], b[..., 0])
    gap = int(np.abs(b[..., 1] - 2 * a[..., 1]).max())
    print("N", n, "largest |G' - 2G|", gap)
    assert gap <= n


def test_views_of_any_layout_get_dense_copies():
    from dct_amd import hip_ops as K
    views, gt = noise_case(25, 3, 12, 10, 4, 2)
    betas = candidates(3, 4)
    want, n = run(views, gt, betas)
    zs, g, bt = [dev(v, np.float32) for v in views], dev(gt, np.int64), dev(betas, np.float32)
    part = K.temperature_sums([z[1:] for z in zs], g[1:], bt, with_ensemble=True)
    assert np.array_equal(part[0].cpu().numpy(), run([v[1:] for v in views], gt[1:], betas)[0])
    nchw = [z.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1) for z in zs]
    got = K.temperature_sums(nchw, g.to(torch.int32), bt.double(), with_ensemble=True)
    assert np.array_equal(got[0].cpu().numpy(), want) and int(got[1].cpu()) == n


# ------------------------------------------------------------------------------------------------------------------ the apply
@pytest.mark.parametrize("B,H,W,C,S", [(1, 1, 1, 2, 1), (3, 37, 53, 3, 2), (1, 130, 130, 4, 2), (2, 9, 11, 8, 8), (2, 9, 11, 2, 4)])
def test_applied_probabilities_against_float64(B, H, W, C, S):
    from dct_amd import hip_ops as K
    views, _ = noise_case(300 + C + S, B, H, W, C, S)
    views = [np.clip(v, -8, 8) for v in views]
    betas = [(0.5, 2.0, 1.5, 1.0)[r % 4] for r in range(S + 1)]
    outs = K.temperature_apply([dev(v, np.float32) for v in views], betas, with_ensemble=True)
    assert len(outs) == S + 1 and all(o.dtype == torch.float32 and tuple(o.shape) == (B, H, W, C) for o in outs)
    ref = applied(flat(views), betas, with_ensemble=True).reshape(S + 1, B, H, W, C)
    d = max(float(np.abs(o.cpu().numpy() - ref[r]).max()) for r, o in enumerate(outs))
    print(f"APPLY {B}x{H}x{W}x{C} S={S}: {d:.3e}")
    assert d <= APPLY_TOL
    alone = K.temperature_apply([dev(v, np.float32) for v in views], betas[:S], with_ensemble=False)
    assert len(alone) == S and all(torch.equal(a, o) for a, o in zip(alone, outs))


@pytest.mark.parametrize("C,S", [(4, 2), (3, 3), (2, 1), (8, 5)])
def test_applied_at_beta_one_is_the_calibration_kernels_softmax(C, S):
    """The reliability tables, Brier and NLL sums of the applied view probabilities are those CalibrationMeter(from_logits=True) counts
    from the logits themselves, cell for cell."""
    from dct_amd.metrics import CalibrationMeter, TemperatureScaler
    views, gt = noise_case(400 + C, 2, 37, 53, C, S)
    zs = [dev(v, np.float32).permute(0, 3, 1, 2) for v in views]
    g = dev(gt, np.int64).unsqueeze(1)
    s = TemperatureScaler(C=C, n_models=S, with_ensemble=True).set_temperature([1.0] * (S + 1))
    probs = s.apply(zs)
    assert len(probs) == S + 1 and tuple(probs[0].shape) == (2, C, 37, 53)
    a = CalibrationMeter(method='2d', C=C, n_models=S, with_ensemble=False, from_logits=True)
    b = CalibrationMeter(method='2d', C=C, n_models=S, with_ensemble=False, from_logits=False)
    a.add(zs, g)
    b.add(probs[:S], g)
    assert np.array_equal(a._rows()[0], b._rows()[0]) and np.array_equal(a._rows()[1], b._rows()[1])
    assert int(a.tables()[..., 0].sum()) == S * 2 * 37 * 53


# --------------------------------------------------------------------------------------------------------------------- the fit
def _batches_of(views, gt, H, W, parts):
    """views [1, N, C] with N = parts * B * H * W -> ``parts`` batches (list of logits [B,C,H,W], gt [B,1,H,W]) on the device."""
    C = views[0].shape[-1]
    zs = [dev(v.reshape(parts, -1, H, W, C), np.float32) for v in views]
    g = dev(gt.reshape(parts, -1, 1, H, W), np.int64)
    return [([z[i].permute(0, 3, 1, 2) for z in zs], g[i]) for i in range(parts)]


def test_fit_against_the_float64_reference_fit():
    """Labels sampled from softmax(z0), the views 3 z0 and z0 / 2: T = 3 and T = 1 / 2 up to the sampling noise, and the device fit
    within FIT_TOL of the same solver on the float64 reference (candidates rounded to fp32 there as well)."""
    from dct_amd.metrics import TemperatureScaler, solve_temperature
    scales = [3.0, 0.5]
    views, gt = sampled_case(31, 2 * 2 * 32 * 32, 4, scales)
    walks = []

    class Walks(list):
        def __iter__(self):
            walks.append(1)
            return super().__iter__()

    s = TemperatureScaler(C=4, n_models=2, with_ensemble=True).fit(Walks(_batches_of(views, gt, 32, 32, 2)))
    assert len(walks) == 5                                      # rounds + 1
    ref = solve_temperature(sum_fn_of(views, gt, with_ensemble=True, fp32_betas=True), 3)
    d = float(np.abs(np.log(s.beta.numpy()) - np.log(ref["beta"])).max())
    print(f"FITDEV {d:.3e} beta {s.beta.tolist()} ref {ref['beta'].tolist()} nll {s.nll_before.tolist()} -> {s.nll_after.tolist()}")
    assert d <= FIT_TOL
    assert s.at_bound == [None] * 3 and all(abs(a * float(s.beta[r]) - 1) < 0.1 for r, a in enumerate(scales))
    assert (s.nll_after.numpy() <= s.nll_before.numpy()).all()
    assert np.abs(s.nll_after.numpy() - ref["nll_after"]).max() <= SUMS_TOL["NLL"]
    t, nll = s.curve()
    assert tuple(t.shape) == (3, 16) and np.abs(nll.numpy() - ref["curve_nll"]).max() <= SUMS_TOL["NLL"]
    # both views scaled back to z0 (each a beta within 0.1 of 1, |z0| < 5: the logits within 1, a probability within 0.25)
    probs = s.apply(_batches_of(views, gt, 32, 32, 2)[0][0])
    assert float((probs[0] - probs[1]).abs().max()) < 0.25


def test_fit_at_the_bounds():
    from dct_amd.metrics import TemperatureScaler
    views, gt = sampled_case(32, 2 * 32 * 32, 4, [64.0, 1 / 64])
    low = TemperatureScaler(C=4, n_models=1, with_ensemble=False).fit(_batches_of(views[:1], gt, 32, 32, 1))
    assert low.at_bound == ['low'] and float(low.temperature[0]) == 16 and float(low.nll_after[0]) <= float(low.nll_before[0])
    hard = views[1].argmax(-1)
    high = TemperatureScaler(C=4, n_models=1, with_ensemble=False).fit(_batches_of(views[1:], hard, 32, 32, 1))
    assert high.at_bound == ['high'] and float(high.temperature[0]) == 1 / 16 and float(high.nll_after[0]) <= float(high.nll_before[0])


# ------------------------------------------------------------------------------------------------------------ through summarize
def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b or (a != a and b != b)


def _segmentators(C, n=2, logit_scale=1.0):
    from dct_amd.models import Segmentator
    segs = []
    for seed in range(n):
        torch.manual_seed(40 + seed)
        seg = Segmentator({"name": "enet", "num_classes": C, "compute_dtype": torch.float32}, {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4},
                          {"name": "StepLR", "step_size": 90, "gamma": 0.1})
        if logit_scale != 1.0:                                  # the classifier is the last transposed convolution: logits x scale
            head = [m for m in seg.torchnet.modules() if type(m).__name__ == "_EConvT"][-1]
            with torch.no_grad():
                for p in head.parameters():
                    p.mul_(logit_scale)
        segs.append(seg)
    return segs


def test_summarize_with_a_fitted_temperature():
    from dct_amd import summary
    C, H, nb = 3, 32, 10
    models = _segmentators(C, logit_scale=3.0)
    val = FakeLoader(batches(91, 4, 1, H, C), 1)
    held = FakeLoader(batches(92, 3, 2, H, C), 2)
    # every class counts: the labels are random, so whatever confidence a network has is over-confidence
    kw = dict(report_axises=[1, 2], kappa=True, calibration=True, calibration_bins=nb)
    plain = summary.summarize(models, val, DEV, "soft", **kw)
    res = summary.summarize(models, val, DEV, "soft", temperature='fit', **kw)
    new = ["calibration_2d_ts", "calibration_3d_ts", "reliability_ts", "temperature"]
    assert sorted(res) == sorted(list(plain) + new)
    assert _same({k: res[k] for k in plain}, plain)             # every table from before is what it was
    keys = ["model_0", "model_1", "ensemble"]
    t = res["temperature"]
    assert list(t) == keys + ["fitted_on", "curve"] and t["fitted_on"] == "val_dataloader"
    assert all(list(t[k]) == ["T", "NLL_before", "NLL_after", "at_bound"] for k in keys)
    assert list(t["curve"]) == keys and len(t["curve"]["ensemble"]["T"]) == len(t["curve"]["ensemble"]["NLL"]) == 16
    for method in ("2d", "3d"):
        assert list(res[f"calibration_{method}_ts"]) == list(res[f"calibration_{method}"])
    assert list(res["reliability_ts"]) == keys and len(res["reliability_ts"]["ensemble"]["count"]) == nb
    assert res["reliability_ts"]["model_0"]["coverage"][0] == 1.0
    print(t["model_0"], t["model_1"], t["ensemble"], res["calibration_3d"], res["calibration_3d_ts"])
    for k in keys:
        assert t[k]["NLL_after"] <= t[k]["NLL_before"]
    for k in keys[:2]:                                          # logits x 3 on random labels: over-confident
        assert t[k]["T"] > 1 and res["calibration_3d_ts"][k]["ECE"] < res["calibration_3d"][k]["ECE"]
        assert sum(res["reliability_ts"][k]["count"]) == sum(res["reliability"][k]["count"])
    # a held-out loader, given temperatures, and no calibration tables
    other = summary.summarize(models, val, DEV, "soft", temperature='fit', temperature_loader=held, **kw)
    assert other["temperature"]["fitted_on"] == "temperature_loader" and _same({k: other[k] for k in plain}, plain)
    assert other["temperature"]["model_0"]["NLL_before"] != t["model_0"]["NLL_before"]       # another set of pixels
    given = summary.summarize(models, val, DEV, "soft", temperature=[t[k]["T"] for k in keys], **kw)
    assert given["temperature"]["fitted_on"] == "given" and np.isnan(given["temperature"]["ensemble"]["NLL_after"])
    assert all(_same(given[k], res[k]) for k in new[:3])
    bare = summary.summarize(models, val, DEV, "soft", report_axises=[1, 2], temperature='fit', calibration_classes=[1, 2])
    assert sorted(bare) == sorted(["2d", "3d", "temperature"]) and bare["temperature"]["model_0"]["T"] != t["model_0"]["T"]
