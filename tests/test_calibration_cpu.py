"""The rule of ``dct_calibration_counts`` (include/dct.h) as a numpy reference, checked on hand-built cases; the host arithmetic of
``metrics.CalibrationMeter`` / ``ece_of`` against it on made-up integer tables; the refusals of the C entry point, which are all
decided before anything is launched and so need no GPU.

The reference has two precisions.  ``exact=True`` follows the kernel's fp32 steps where they decide an integer: the ensemble mean
(summed in view order, one division), the bin (one fp32 multiply) and the 2^24 confidence word; test_calibration_gpu.py compares
those tables with ``np.array_equal``.  ``exact=False`` does everything in float64, softmax included, and also marks the pixels
whose bin or argmax a last-bit difference could move.  Brier and NLL are float64 in both."""
import ctypes

import numpy as np
import pytest
import torch

UNIT = float(1 << 24)


# ------------------------------------------------------------------------------------------------------------------- reference
def rater_probs(views, with_ensemble, from_logits, exact):
    """views: S arrays [B, P, C] -> [R, B, P, C] probabilities, float32 (exact) or float64."""
    dt = np.float32 if exact else np.float64
    ps = []
    for v in views:
        x = np.asarray(v, dtype=np.float32).astype(dt)
        if from_logits:
            e = np.exp(x - x.max(-1, keepdims=True)).astype(dt)
            tot = np.zeros(e.shape[:-1], dtype=dt)
            for c in range(e.shape[-1]):            # in class order
                tot = (tot + e[..., c]).astype(dt)
            x = (e / tot[..., None]).astype(dt)
        ps.append(x)
    if with_ensemble:
        acc = np.zeros_like(ps[0])
        for p in ps:                                # in view order
            acc = (acc + p).astype(dt)
        ps.append((acc / dt(len(views))).astype(dt))
    return np.stack(ps)


def reference(views, gt, n_bins, classes=None, with_ensemble=False, from_logits=False, exact=True):
    """-> dict: bins int64 [B, R, n_bins, 3], brier / nll float64 [B, R] (sums over the counted pixels), N int64 [B], and the
    per-pixel arrays counted [B, P], bin / correct / uncertain [R, B, P]."""
    p = rater_probs(views, with_ensemble, from_logits, exact)
    R, B, P, C = p.shape
    gt = np.asarray(gt).reshape(B, P).astype(np.int64)
    allowed = np.zeros(C, dtype=bool)
    allowed[list(range(C)) if classes is None else list(classes)] = True
    valid = (gt >= 0) & (gt < C)
    t = np.where(valid, gt, 0)
    counted = valid & allowed[t]
    conf = p.max(-1)
    pred = p.argmax(-1)                             # first maximum
    scaled = (conf * np.float32(n_bins)).astype(np.float32) if exact else conf * n_bins
    word = np.floor(conf.astype(np.float64) * UNIT).astype(np.int64)            # conf * 2^24 is exact in fp32: the cast truncates
    bin_ = np.minimum(n_bins - 1, np.floor(scaled).astype(np.int64))
    correct = pred == t[None]
    p64 = p.astype(np.float64)
    onehot = np.eye(C)[t]
    brier_px = ((p64 - onehot[None]) ** 2).sum(-1)
    nll_px = -np.log(np.take_along_axis(p64, np.broadcast_to(t[None, ..., None], (R, B, P, 1)), -1)[..., 0] + 1e-10)
    near = np.rint(scaled)
    srt = np.sort(p64, -1)
    uncertain = ((np.abs(scaled - near) < 1e-4) & (near >= 1) & (near <= n_bins - 1))
    if C > 1:
        uncertain = uncertain | (srt[..., -1] - srt[..., -2] < 1e-5)
    bins = np.zeros((B, R, n_bins, 3), dtype=np.int64)
    for r in range(R):
        for b in range(B):
            m = counted[b]
            k = bin_[r, b][m]
            bins[b, r, :, 0] = np.bincount(k, minlength=n_bins)
            bins[b, r, :, 1] = np.bincount(k, weights=correct[r, b][m], minlength=n_bins).astype(np.int64)
            np.add.at(bins[b, r, :, 2], k, word[r, b][m])
    w = counted[None].astype(np.float64)
    return dict(bins=bins, brier=(brier_px * w).sum(-1).T, nll=(nll_px * w).sum(-1).T, N=counted.sum(-1), counted=counted, bin=bin_,
                correct=correct, uncertain=uncertain, conf=conf)


def derived(bins, brier=None, nll=None):
    """ECE, MCE (and mean Brier, mean NLL) of tables [..., n_bins, 3] in float64, by the formulas of include/dct.h, bin by bin."""
    bins = np.asarray(bins, dtype=np.float64)
    lead = bins.shape[:-2]
    flat = bins.reshape(-1, bins.shape[-2], 3)
    ece, mce = np.full(len(flat), np.nan), np.full(len(flat), np.nan)
    for i, tab in enumerate(flat):
        N = tab[:, 0].sum()
        if N == 0:
            continue
        gaps = [(n / N, abs(c / n - s / (UNIT * n))) for n, c, s in tab if n > 0]
        ece[i] = sum(wt * g for wt, g in gaps)
        mce[i] = max(g for _, g in gaps)
    out = [ece.reshape(lead), mce.reshape(lead)]
    N = bins[..., 0].sum(-1)
    for v in (brier, nll):
        if v is not None:
            with np.errstate(divide='ignore', invalid='ignore'):
                out.append(np.where(N > 0, np.asarray(v, dtype=np.float64) / N, np.nan))
    return out


def noise_probs(rng, B, P, C, sharp=2.0):
    x = rng.normal(0, sharp, (B, P, C))
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------- the reference itself
def test_reference_on_hand_built_pixels():
    # one image, four pixels, C = 2, n_bins = 4: conf 0.9 right, 0.9 wrong, 0.6 right, and one with gt = 255
    p = np.array([[[0.9, 0.1], [0.9, 0.1], [0.4, 0.6], [0.7, 0.3]]], dtype=np.float32)
    gt = np.array([[0, 1, 1, 255]])
    r = reference([p], gt, 4)
    w9, w6 = int(np.float32(0.9) * UNIT), int(np.float32(0.6) * UNIT)
    assert r["bins"].tolist() == [[[[0, 0, 0], [0, 0, 0], [1, 1, w6], [2, 1, 2 * w9]]]]
    assert r["N"].tolist() == [3]
    f = lambda a: float(np.float32(a))
    assert np.isclose(r["brier"][0, 0], 2 * f(.1) ** 2 + 2 * f(.9) ** 2 + 2 * f(.4) ** 2, rtol=1e-6)
    assert np.isclose(r["nll"][0, 0], -np.log(f(.9)) - np.log(f(.1)) - np.log(f(.6)), rtol=1e-6)
    ece, mce, brier, nll = derived(r["bins"], r["brier"], r["nll"])
    assert np.isclose(ece[0, 0], (1 / 3) * abs(1 - f(.6)) + (2 / 3) * abs(.5 - f(.9)), atol=1e-7)
    assert np.isclose(mce[0, 0], abs(.5 - f(.9)), atol=1e-7) and np.isclose(brier[0, 0], r["brier"][0, 0] / 3)


def test_reference_edges_ties_mask_and_ensemble():
    # conf * n_bins exactly 1.0 lands in bin 1; conf = 1.0 in the last bin; an exact tie goes to the first class
    quarter = np.full((1, 3, 4), 0.25, dtype=np.float32)
    r = reference([quarter], np.array([[0, 1, 3]]), 4)
    assert r["bins"][0, 0, :, 0].tolist() == [0, 3, 0, 0] and r["bins"][0, 0, 1, 1] == 1
    one = np.eye(4, dtype=np.float32)[None, [2, 0, 1]]
    r = reference([one], np.array([[2, 0, 3]]), 4)
    assert r["bins"][0, 0, 3].tolist() == [3, 2, 3 << 24] and np.isclose(r["nll"][0, 0], -np.log(1e-10))
    # the class mask is the same as dropping the pixels; gt outside [0, C) never counts
    rng = np.random.default_rng(0)
    p, gt = noise_probs(rng, 2, 50, 3), rng.integers(0, 3, (2, 50))
    gt[0, :5] = (255, -1, 3, 255, -1)
    masked = reference([p], gt, 10, classes=[1, 2])
    assert np.array_equal(masked["bins"], reference([p], np.where(gt == 0, 255, gt), 10)["bins"])
    assert masked["N"].tolist() == [int(((gt[b] == 1) | (gt[b] == 2)).sum()) for b in range(2)]
    # the ensemble is the last rater, the mean in fp32; with one view it is that view
    q = noise_probs(rng, 2, 50, 3)
    r = reference([p, q], gt, 10, with_ensemble=True)
    assert r["bins"].shape == (2, 3, 10, 3)
    assert np.array_equal(r["bins"][:, 2], reference([((p + q) / np.float32(2)).astype(np.float32)], gt, 10)["bins"][:, 0])
    r1 = reference([p], gt, 10, with_ensemble=True)
    assert np.array_equal(r1["bins"][:, 0], r1["bins"][:, 1])
    # float64 logits mode agrees with the fp32 one but for the uncertain pixels
    x = rng.normal(0, 2, (2, 400, 4)).astype(np.float32)
    g = rng.integers(0, 4, (2, 400))
    a, b = reference([x], g, 15, from_logits=True, exact=True), reference([x], g, 15, from_logits=True, exact=False)
    assert (np.abs(a["bins"][..., :2] - b["bins"][..., :2]).sum() <= 2 * b["uncertain"].sum()) and b["uncertain"].mean() < 0.01


def test_confidence_word_stays_within_2_pow_minus_24():
    conf = np.random.default_rng(1).random(1_000_000).astype(np.float32)
    word = np.floor(conf.astype(np.float64) * UNIT)
    assert (np.float32(conf * np.float32(UNIT)) == conf.astype(np.float64) * UNIT).all()          # the scaling itself is exact
    err = conf.astype(np.float64) - word / UNIT
    assert err.min() >= 0 and err.max() < 2.0 ** -24 and (err[conf >= 0.5] == 0).all()


# ------------------------------------------------------------------------------------------------------------- host arithmetic
def test_ece_of_textbook_example():
    """Three bins of ten: 100 predictions at confidence 0.55 of which 60 are right, 300 at 0.75 with 210 right, 600 at 0.95 with 540
    right; seven bins stay empty.  ECE = 0.1 * 0.05 + 0.3 * 0.05 + 0.6 * 0.05 = 0.05; MCE = 0.05."""
    from dct_amd.metrics import ece_of, mce_of
    bins = np.zeros((10, 3), dtype=np.int64)
    for k, n, right, conf in ((5, 100, 60, 0.55), (7, 300, 210, 0.75), (9, 600, 540, 0.95)):
        bins[k] = (n, right, n * int(conf * UNIT))
    assert abs(float(ece_of(bins)) - 0.05) < 1e-6 and abs(float(mce_of(bins)) - 0.05) < 1e-6
    bins[9] = (600, 570, 600 * int(0.95 * UNIT))            # the top bin now calibrated: 0.1 * 0.05 + 0.3 * 0.05
    assert abs(float(ece_of(bins)) - 0.02) < 1e-6 and abs(float(mce_of(bins)) - 0.05) < 1e-6
    stack = np.stack([bins, np.zeros_like(bins)])
    got = ece_of(stack)
    assert got.shape == (2,) and np.isnan(got[1]) and np.isnan(mce_of(stack)[1])
    np.testing.assert_allclose(ece_of(stack), derived(stack)[0], rtol=1e-14, equal_nan=True)


def _filled_meter(method, rows_bins, rows_scores, **kw):
    """A meter whose log holds made-up integer rows (the host arithmetic needs no device)."""
    from dct_amd.metrics import CalibrationMeter
    m = CalibrationMeter(method=method, **kw)
    b, s = torch.from_numpy(rows_bins), torch.from_numpy(rows_scores)
    m.countLog.append(torch.cat((b.flatten(2), s), dim=2))
    return m


def test_meter_host_arithmetic_on_made_up_tables():
    rng = np.random.default_rng(5)
    rows, R, nb = 6, 3, 8
    n = rng.integers(0, 50, (rows, R, nb))
    n[:, :, 2] = 0                                  # an empty bin everywhere
    n[3] = 0                                        # a row with N = 0
    n[4, 1] = 0                                     # ... and one rater of another row
    right = (n * rng.random((rows, R, nb))).astype(np.int64)
    conf = (n * (rng.random((rows, R, nb)) * UNIT).astype(np.int64))
    bins = np.stack([n, right, conf], -1).astype(np.int64)
    N = n.sum(-1)
    scores = np.stack([(N * rng.random((rows, R)) * UNIT).astype(np.int64), (N * 3 * rng.random((rows, R)) * UNIT).astype(np.int64)], -1)
    m = _filled_meter('2d', bins, scores, C=4, n_models=2, with_ensemble=True, n_bins=nb)
    assert m.raters == ["S0", "S1", "ensemble"]
    ece, mce, brier, nll = derived(bins, scores[..., 0] / UNIT, scores[..., 1] / UNIT)
    assert np.isnan(ece[3]).all() and np.isnan(ece[4, 1]) and not np.isnan(ece[4, 0])
    for got, ref in ((m.ece(), ece), (m.mce(), mce), (m.brier(), brier), (m.nll(), nll)):
        mean, std, defined = (x.numpy() for x in got)
        assert defined.tolist() == [5, 4, 5]
        for r in range(R):
            col = ref[:, r][~np.isnan(ref[:, r])]
            assert np.isclose(mean[r], col.mean(), rtol=1e-12) and np.isclose(std[r], col.std(ddof=1), rtol=1e-10)
    with np.errstate(invalid='ignore'):
        rep = np.array([np.nanmean(ece[i]) for i in range(rows) if not np.isnan(ece[i]).all()])
    s = m.summary()
    assert list(s) == ['mECE', 'mVars'] and np.isclose(s['mECE'], rep.mean(), rtol=1e-12) and np.isclose(s['mVars'], rep.std(ddof=1), rtol=1e-10)
    assert np.isclose(m.value()[0][0], rep.mean(), rtol=1e-12) and np.allclose(m.value()[1][0].numpy(), m.ece()[0].numpy())
    d = m.detailed_summary()
    assert list(d) == m.raters and list(d["S0"]) == ['ECE', 'MCE', 'Brier', 'NLL'] and d["ensemble"]["NLL"] == float(m.nll()[0][2])
    # pooled readers
    pooled = bins.sum(0)
    assert np.array_equal(m.tables().numpy(), pooled)
    count, acc, cf = (x.numpy() for x in m.reliability())
    assert np.array_equal(count, pooled[..., 0]) and np.isnan(acc[:, 2]).all() and np.isnan(cf[:, 2]).all()
    ok = pooled[..., 0] > 0
    assert np.allclose(acc[ok], pooled[..., 1][ok] / pooled[..., 0][ok], rtol=1e-14)
    assert np.allclose(cf[ok], pooled[..., 2][ok] / UNIT / pooled[..., 0][ok], rtol=1e-14)
    cov, kept = (x.numpy() for x in m.coverage_accuracy())
    for r in range(R):
        for k in range(nb):
            tail = pooled[r, k:]
            assert np.isclose(cov[r, k], tail[:, 0].sum() / pooled[r, :, 0].sum(), rtol=1e-14)
            assert np.isclose(kept[r, k], tail[:, 1].sum() / tail[:, 0].sum(), rtol=1e-14)
    assert (cov[:, 0] == 1.0).all() and (np.diff(cov, axis=1) <= 0).all()


def test_meter_with_nothing_added_or_counted():
    from dct_amd.metrics import CalibrationMeter
    m = CalibrationMeter(method='3d', C=3, n_models=2, with_ensemble=False, n_bins=5, rater_names=["a", "b"])
    assert m.raters == ["a", "b"]
    for got in (m.ece(), m.mce(), m.brier(), m.nll()):
        assert np.isnan(got[0].numpy()).all() and np.isnan(got[1].numpy()).all() and got[2].tolist() == [0, 0]
    assert np.isnan(m.summary()['mECE']) and int(m.tables().sum()) == 0 and tuple(m.tables().shape) == (2, 5, 3)
    count, acc, cf = m.reliability()
    assert int(count.sum()) == 0 and np.isnan(acc.numpy()).all() and np.isnan(cf.numpy()).all()
    cov, kept = m.coverage_accuracy()
    assert np.isnan(cov.numpy()).all() and np.isnan(kept.numpy()).all()
    z = _filled_meter('2d', np.zeros((2, 2, 5, 3), dtype=np.int64), np.zeros((2, 2, 2), dtype=np.int64), C=3, n_models=2, with_ensemble=False,
                      n_bins=5)
    assert z.ece()[2].tolist() == [0, 0] and np.isnan(z.detailed_summary()["S1"]["Brier"])


def test_meter_refuses_cpu_tensors_and_wrong_lists():
    from dct_amd import hip_ops as K
    from dct_amd import metrics as M
    assert {"CalibrationMeter", "ece_of"} <= set(M.__all__)
    m = M.CalibrationMeter(method='2d', C=3, n_models=2)
    p, gt = torch.full((1, 3, 4, 4), 1 / 3), torch.zeros(1, 1, 4, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.add([p, p], gt)
    with pytest.raises(RuntimeError, match="list of 2 predictions"):
        m.add([p], gt)
    with pytest.raises(RuntimeError, match="list of 2 predictions"):
        m.add(p, gt)
    with pytest.raises(RuntimeError, match="gt is required"):
        m.add([p, p], None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.calibration_counts([p.permute(0, 2, 3, 1)], gt.reshape(1, -1))
    with pytest.raises(ValueError):
        K.calibration_counts([], gt)
    with pytest.raises(ValueError, match="classes"):
        K.calibration_counts([p.permute(0, 2, 3, 1)], gt.reshape(1, -1), classes=[3])
    with pytest.raises(AssertionError):
        M.CalibrationMeter(n_bins=33)
    with pytest.raises(AssertionError):
        M.CalibrationMeter(n_models=9)


def test_switches_default_to_off():
    import inspect
    from dct_amd import summary
    from dct_amd.trainer import CoTrainer
    p = inspect.signature(summary.summarize).parameters
    assert list(p)[-3:] == ["calibration", "calibration_bins", "calibration_classes"]
    assert p["calibration"].default is False and p["calibration_bins"].default == 15 and p["calibration_classes"].default is None
    q = inspect.signature(CoTrainer.__init__).parameters
    assert list(q)[-1] == "val_calibration" and q["val_calibration"].default is False
    m = inspect.signature(__import__("dct_amd.metrics", fromlist=["x"]).CalibrationMeter.__init__).parameters
    assert list(m)[1:] == ["method", "C", "n_models", "with_ensemble", "n_bins", "considered_classes", "from_logits", "rater_names"]


# ------------------------------------------------------------------------------------------------------------- the entry point
def test_entry_point_refuses_before_it_launches():
    """Every call here is refused on its arguments alone (made-up addresses are never dereferenced on the device: nothing is
    launched), so the statuses can be read without a GPU."""
    from dct_amd import _lib
    fn = _lib.load().dct_calibration_counts
    BAD, UNSUPPORTED = -1, _lib.ERR_UNSUPPORTED      # DCT_ERR_BAD_ARG, DCT_ERR_UNSUPPORTED

    def status(S=2, C=4, B=2, ppi=100, n_bins=15, gt=0x2000, bins=0x3000, scores=0x4000, entries=None, probs="array", ens=1, logits=0):
        entries = [0x10000 + 0x1000 * s for s in range(max(S, 1))] if entries is None else entries
        arr = (ctypes.c_void_p * len(entries))(*entries)
        return fn(arr if probs == "array" else None, S, gt, B, ppi, C, n_bins, 0xFF, ens, logits, bins, scores, None)

    for kw in (dict(probs=None), dict(gt=0), dict(bins=0), dict(scores=0), dict(S=0), dict(S=-1), dict(B=0), dict(ppi=0),
               dict(entries=[0x10000, 0]), dict(ens=2), dict(logits=-1),
               dict(C=4, entries=[0x10000, 0x11008]), dict(C=2, entries=[0x10000, 0x11004]), dict(C=3, entries=[0x10000, 0x11002]),
               dict(gt=0x2004), dict(bins=0x3004), dict(scores=0x4004)):
        assert status(**kw) == BAD, kw
    for kw in (dict(S=9, entries=[0x10000] * 9), dict(C=0), dict(C=9), dict(n_bins=0), dict(n_bins=33), dict(B=65536), dict(ppi=1 << 31)):
        assert status(**kw) == UNSUPPORTED, kw
