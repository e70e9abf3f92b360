"""Temperature scaling without a device: the numpy reference of the rule (temperature_ref.py) on hand-built pixels,
``metrics.solve_temperature`` on that reference against a bisection to convergence, the exact scaling property of the rule in fp32, the
host arithmetic of ``metrics.TemperatureScaler`` on made-up integer sums, and the refusals of the two C entry points, which are all
decided before anything is launched."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from temperature_ref import UNIT, applied, pixel_terms, rater_logits, reference, sampled_case, sum_fn_of, words


# ------------------------------------------------------------------------------------------------------- the reference itself
def test_reference_on_hand_built_pixels():
    # one image, four pixels, C = 2: logits (2, 0) with gt 0, (2, 0) with gt 1, (0, 1) with gt 1, and one with gt = 255
    z = np.array([[[2., 0.], [2., 0.], [0., 1.], [5., 5.]]], dtype=np.float32)
    gt = np.array([[0, 1, 1, 255]])
    r = reference([z], gt, np.array([[1.0, 0.5]]))
    assert r["N"] == 3
    sp = lambda d: np.log1p(np.exp(-d))                          # nll of the class that leads by d
    for k, b in enumerate((1.0, 0.5)):
        nll = sp(2 * b) + (sp(2 * b) + 2 * b) + sp(b)
        # g = E_p[z] - z_y: p = sigmoid(+-d)
        p0, q1 = 1 / (1 + np.exp(-2 * b)), 1 / (1 + np.exp(-b))
        g = (2 * p0 - 2) + (2 * p0 - 0) + (q1 - 1)
        assert np.isclose(r["nll"][0, k], nll, rtol=1e-12) and np.isclose(r["g"][0, k], g, rtol=1e-12)
        assert abs(r["sums"][0, k, 0] - nll * UNIT) <= 1.5 and abs(r["sums"][0, k, 1] - g * UNIT) <= 1.5
    # g is the derivative of nll in beta
    h = 1e-6
    d = reference([z], gt, np.array([[0.7 - h, 0.7, 0.7 + h]]))
    assert np.isclose((d["nll"][0, 2] - d["nll"][0, 0]) / (2 * h), d["g"][0, 1], rtol=1e-6)
    # and non-decreasing in beta
    grid = reference([z], gt, np.exp2(np.linspace(-4, 4, 16))[None])
    assert (np.diff(grid["g"][0]) >= 0).all()


def test_reference_words_clamp_and_drop_nan():
    nll = np.array([0.0, 1.0, 5000.0, np.inf, np.nan, 2.0 ** -21, 3 * 2.0 ** -21])
    g = np.array([0.0, -1.5, 3000.0, -np.inf, np.nan, 2.0 ** -21, -3 * 2.0 ** -21])
    wn, wg = words(nll, g)
    assert wn.tolist() == [0, 1 << 20, 4095 << 20, 4095 << 20, 0, 0, 2]           # ties to even
    assert wg.tolist() == [0, -3 << 19, 2047 << 20, -(2047 << 20), 0, 0, -2]


def test_reference_mask_invalid_gt_and_ensemble():
    rng = np.random.default_rng(0)
    z, w = (rng.normal(0, 2, (2, 50, 3)).astype(np.float32) for _ in range(2))
    gt = rng.integers(0, 3, (2, 50))
    gt[0, :5] = (255, -1, 3, 255, -1)
    betas = np.tile(np.array([0.5, 1.0, 2.0]), (3, 1))
    masked = reference([z, w], gt, betas, classes=[1, 2], with_ensemble=True)
    dropped = reference([z, w], np.where(gt == 0, 255, gt), betas, with_ensemble=True)
    assert np.array_equal(masked["sums"], dropped["sums"]) and masked["N"] == dropped["N"] == int(((gt == 1) | (gt == 2)).sum())
    # the ensemble rater: log of the mean of the two softmaxes; at beta = 1 its nll is the calibration rule's -log(p_gt + 1e-10)
    u = rater_logits([z, w], True, False)
    p = [np.exp(v - v.max(-1, keepdims=True)) / np.exp(v - v.max(-1, keepdims=True)).sum(-1, keepdims=True) for v in (z.astype(np.float64), w.astype(np.float64))]
    assert u.shape == (3, 2, 50, 3) and np.allclose(u[2], np.log((p[0] + p[1]) / 2 + 1e-10), rtol=0, atol=1e-12)
    ok = (gt >= 0) & (gt < 3)
    pe = ((p[0] + p[1]) / 2)[ok, gt[ok]]
    full = reference([z, w], gt, betas, with_ensemble=True)
    assert np.isclose(full["nll"][2, 1], -np.log(pe + 1e-10).sum() + np.log((np.exp(u[2]).sum(-1))[ok]).sum(), rtol=1e-10)
    # the fp32 variant forms the mean as the calibration rule does: fp32 sums in view order, one division; then one fp32 log
    u32 = rater_logits([z, w], True, True)
    assert u32.dtype == np.float32 and np.abs(u32[2] - u[2]).max() < 2e-6
    # one view: the ensemble is log softmax of it, and scaling it by beta = 1 gives the view's own nll
    one = reference([z], gt, np.ones((2, 1)), with_ensemble=True)
    assert abs(one["nll"][0, 0] - one["nll"][1, 0]) < 1e-6 * one["N"]
    # applied probabilities: softmax(beta z), rows sum to one
    a = applied([z, w], [0.5, 2.0, 1.0], with_ensemble=True)
    assert a.shape == (3, 2, 50, 3) and np.allclose(a.sum(-1), 1) and np.allclose(a[2], np.exp(u[2]) / np.exp(u[2]).sum(-1, keepdims=True))


# ------------------------------------------------------------------------------------------------------------------ the solver
def bisect_log_beta(fn, lo=-4.0, hi=4.0):
    """The root of a rater's gradient sum ``fn(log2 beta)`` by bisection to convergence (the same integer sums, one candidate a call)."""
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if mid in (lo, hi):
            break
        if fn(mid) <= 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def grad_at(views, gt, r, with_ensemble=False):
    R = len(views) + int(with_ensemble)

    def fn(log2_beta):
        betas = np.ones((R, 1))
        betas[r, 0] = np.exp2(log2_beta)
        return reference(views, gt, betas, with_ensemble=with_ensemble)["sums"][r, 0, 1]
    return fn


@pytest.mark.parametrize("sigma", [1.0, 2.0])
def test_solver_agrees_with_a_bisection_and_recovers_the_scale(sigma):
    """Labels sampled from softmax(z0), logits a z0: the calibrated inverse temperature is 1 / a.  Observed at N = 8192, C = 4, a = 3:
    a beta = 0.986 and 0.987, the secant within 2.3e-9 and 1.0e-8 of the bisection in log2 beta (asserted: 1e-6 in ln beta)."""
    from dct_amd.metrics import solve_temperature
    a = 3.0
    views, gt = sampled_case(5 + int(sigma), 8192, 4, [a], sigma)
    calls = []

    def fn(betas):
        calls.append(np.array(betas))
        return sum_fn_of(views, gt)(betas)
    fit = solve_temperature(fn, 1)
    assert len(calls) == 5 and [c.shape for c in calls] == [(1, 16)] * 4 + [(1, 2)]
    assert calls[0][0, 0] == 2.0 ** -4 and calls[0][0, -1] == 2.0 ** 4 and calls[4][0, 0] == 1.0 and calls[4][0, 1] == fit["beta"][0]
    root = bisect_log_beta(grad_at(views, gt, 0))
    print(f"sigma {sigma}: a * beta {a * fit['beta'][0]:.4f}, |log2 beta - bisection| {abs(np.log2(fit['beta'][0]) - root):.3e}")
    assert abs(np.log(fit["beta"][0]) - root * np.log(2)) <= 1e-6
    assert abs(a * fit["beta"][0] - 1) < 0.1
    assert fit["at_bound"] == [None] and fit["N"] == 8192 and np.isclose(fit["temperature"][0], 1 / fit["beta"][0])
    assert fit["nll_after"][0] < fit["nll_before"][0]
    # the curve: the first grid, from T = 16 down to 1 / 16, its minimum next to the fit
    assert fit["curve_temperature"].shape == (1, 16) and fit["curve_temperature"][0, 0] == 16 and fit["curve_temperature"][0, -1] == 1 / 16
    k = int(fit["curve_nll"][0].argmin())
    assert fit["curve_temperature"][0, min(k + 1, 15)] <= fit["temperature"][0] <= fit["curve_temperature"][0, max(k - 1, 0)]
    assert fit["nll_after"][0] <= fit["curve_nll"][0].min() + 1e-9


@pytest.mark.parametrize("S,C,ens", [(1, 2, False), (2, 4, True), (3, 3, True), (4, 8, False)])
def test_solver_on_several_raters_at_once(S, C, ens):
    """Mixed scales: every rater gets its own bracket; the ensemble's root is a number of its own."""
    from dct_amd.metrics import solve_temperature
    scales = [0.5, 1.0, 3.0, 5.0][:S]
    views, gt = sampled_case(40 + S, 4096, C, scales)
    R = S + int(ens)
    fit = solve_temperature(sum_fn_of(views, gt, with_ensemble=ens), R)
    for r in range(R):
        root = bisect_log_beta(grad_at(views, gt, r, ens))
        assert abs(np.log(fit["beta"][r]) - root * np.log(2)) <= 1e-6, r
    for r, a in enumerate(scales):
        assert abs(a * fit["beta"][r] - 1) < 0.1, (r, a, fit["beta"][r])
    assert fit["at_bound"] == [None] * R and (fit["nll_after"] <= fit["nll_before"]).all()
    print(S, C, fit["beta"])


def test_solver_bounds_and_nothing_counted():
    from dct_amd.metrics import solve_temperature
    views, gt = sampled_case(9, 2048, 4, [1.0])
    z = views[0]
    # logits x 64: wildly over-confident, the root lies below 1 / 16 -> 'low', T = 16
    low = solve_temperature(sum_fn_of([z * 64], gt), 1)
    assert low["at_bound"] == ['low'] and low["temperature"][0] == 16 and low["beta"][0] == 1 / 16
    # labels = argmax, logits / 64: under-confident and always right, the root lies above 16 -> 'high', T = 1 / 16
    high = solve_temperature(sum_fn_of([z / 64], z.argmax(-1)), 1)
    assert high["at_bound"] == ['high'] and high["temperature"][0] == 1 / 16
    assert high["nll_after"][0] < high["nll_before"][0] and low["nll_after"][0] < low["nll_before"][0]
    # one rater at a bound, the other not
    both = solve_temperature(sum_fn_of([z * 64, 2 * z], gt), 2)
    assert both["at_bound"] == ['low', None] and abs(2 * both["beta"][1] - 1) < 0.1
    # N = 0: NaN, after one call
    calls = []
    none = solve_temperature(lambda b: (calls.append(1), sum_fn_of([z], np.full_like(gt, 255))(b))[1], 1)
    assert len(calls) == 1 and none["N"] == 0 and np.isnan(none["beta"]).all() and np.isnan(none["temperature"]).all()
    assert np.isnan(none["nll_before"]).all() and np.isnan(none["nll_after"]).all() and np.isnan(none["curve_nll"]).all()


# ------------------------------------------------------------------------------------------------------ exact scaling property
def test_doubling_the_logits_and_halving_beta_keeps_the_nll_words():
    """x = beta z is the same number, so every NLL word is; g doubles exactly in fp32, and each of its words is rounded once:
    |G' - 2 G| <= N.  Observed: identical NLL words, 38 <= 2738."""
    rng = np.random.default_rng(12)
    z = rng.normal(0, 2, (2, 1369, 4)).astype(np.float32)
    gt = rng.integers(0, 4, (2, 1369))
    betas = np.exp2(np.linspace(-3, 3, 7)).astype(np.float32)[None]
    a = reference([z], gt, betas, exact=True)
    b = reference([2 * z], gt, betas / 2, exact=True)
    assert np.array_equal(a["sums"][..., 0], b["sums"][..., 0])
    gap = np.abs(b["sums"][..., 1] - 2 * a["sums"][..., 1]).max()
    print("N", a["N"], "largest |G' - 2G|", gap)
    assert gap <= a["N"]
    # and the fp32 rule stays close to the float64 one
    ref = reference([z], gt, betas.astype(np.float64))
    assert np.abs(a["sums"][..., 0] - ref["sums"][..., 0]).max() / (UNIT * a["N"]) < 1e-6
    nll, g = pixel_terms(z[0, :3], gt[0, :3], 1.0, True)
    assert nll.dtype == np.float32 and g.dtype == np.float32


# ------------------------------------------------------------------------------------------------------------- host arithmetic
def made_up_sum_fn(roots, slopes, N, offsets):
    """Integer sums of raters whose gradient is slope * (log2 beta - root) per pixel and whose NLL is the integral of that."""
    def fn(betas):
        lb = np.log2(np.asarray(betas, dtype=np.float64))
        g = slopes[:, None] * (lb - roots[:, None])
        nll = offsets[:, None] + 0.5 * slopes[:, None] * (lb - roots[:, None]) ** 2
        return np.stack([np.rint(nll * N * UNIT), np.rint(g * N * UNIT)], -1).astype(np.int64), N
    return fn


def test_scaler_host_arithmetic_on_made_up_sums():
    from dct_amd import metrics as M
    assert {"TemperatureScaler", "solve_temperature"} <= set(M.__all__)
    roots, slopes, offsets = np.array([-1.234567, 0.5, 9.0]), np.array([0.3, 2.0, 1.0]), np.array([0.7, 0.2, 0.1])
    s = M.TemperatureScaler(C=4, n_models=2, with_ensemble=True, rater_names=["a", "b"])
    assert s.raters == ["a", "b", "ensemble"]
    with pytest.raises(RuntimeError, match="fit"):
        s.temperature
    assert s.fit_sums(made_up_sum_fn(roots, slopes, 1000, offsets)) is s
    # a linear gradient: the secant is exact up to the rounding of the integer sums
    assert np.allclose(np.log2(s.beta.numpy()[:2]), roots[:2], rtol=0, atol=1e-8)
    assert s.at_bound == [None, None, 'high'] and float(s.beta[2]) == 16 and float(s.temperature[2]) == 1 / 16
    assert np.allclose(s.temperature.numpy(), 1 / s.beta.numpy()) and s.temperature.dtype == torch.float64
    assert np.allclose(s.nll_after.numpy()[:2], offsets[:2], atol=1e-6)
    assert np.allclose(s.nll_before.numpy(), offsets + 0.5 * slopes * roots ** 2, atol=1e-6)
    t, nll = s.curve()
    assert tuple(t.shape) == tuple(nll.shape) == (3, 16) and float(t[0, 0]) == 16 and float(t[2, -1]) == 1 / 16
    d = s.detailed_summary()
    assert list(d) == s.raters and list(d["a"]) == ['T', 'NLL_before', 'NLL_after', 'at_bound']
    assert d["ensemble"]["at_bound"] == 'high' and d["a"]["at_bound"] is None and d["b"]["T"] == float(s.temperature[1])
    # other grids: 8 candidates, 6 rounds get as close
    s8 = M.TemperatureScaler(C=4, n_models=2, with_ensemble=True, n_candidates=8, rounds=6).fit_sums(made_up_sum_fn(roots, slopes, 1000, offsets))
    assert np.allclose(np.log2(s8.beta.numpy()[:2]), roots[:2], rtol=0, atol=1e-8)
    # given temperatures
    g = M.TemperatureScaler(C=3, n_models=1, with_ensemble=False).set_temperature([2.0])
    assert g.beta.tolist() == [0.5] and g.at_bound == [None] and np.isnan(g.nll_after.numpy()).all() and tuple(g.curve()[0].shape) == (1, 0)
    with pytest.raises(ValueError):
        g.set_temperature([1.0, 2.0])
    with pytest.raises(ValueError):
        g.set_temperature([0.0])


def test_scaler_and_ops_refuse_cpu_tensors_and_wrong_lists():
    from dct_amd import hip_ops as K
    from dct_amd import metrics as M
    s = M.TemperatureScaler(C=3, n_models=2).set_temperature([1, 1, 1])
    z, gt = torch.zeros(1, 3, 4, 4), torch.zeros(1, 1, 4, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.fit([([z, z], gt)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.apply([z, z])
    with pytest.raises(RuntimeError, match="list of 2 predictions"):
        s.apply([z])
    with pytest.raises(RuntimeError, match="list of 2 predictions"):
        s.fit([([z], gt)])
    nhwc, betas = z.permute(0, 2, 3, 1), torch.ones(1, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.temperature_sums([nhwc], gt.reshape(1, -1), betas)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.temperature_apply([nhwc], [1.0])
    with pytest.raises(ValueError):
        K.temperature_sums([], gt, betas)
    with pytest.raises(ValueError, match="classes"):
        K.temperature_sums([nhwc], gt.reshape(1, -1), betas, classes=[3])
    with pytest.raises(ValueError, match="betas"):
        K.temperature_sums([nhwc], gt.reshape(1, -1), torch.ones(2, 4))
    with pytest.raises(ValueError, match="betas"):
        K.temperature_sums([nhwc], gt.reshape(1, -1), torch.ones(1, 17))
    with pytest.raises(ValueError, match="gt"):
        K.temperature_sums([nhwc], gt.reshape(1, -1)[:, :3], betas)
    with pytest.raises(ValueError, match="inverse temperatures"):
        K.temperature_apply([nhwc], [1.0, 1.0])
    with pytest.raises(AssertionError):
        M.TemperatureScaler(n_models=9)
    with pytest.raises(AssertionError):
        M.TemperatureScaler(n_candidates=17)


def test_new_arguments_default_to_off():
    from dct_amd import summary
    from dct_amd.metrics import TemperatureScaler, solve_temperature
    p = inspect.signature(summary.summarize).parameters
    assert p["temperature"].default is None and p["temperature_loader"].default is None
    q = inspect.signature(TemperatureScaler.__init__).parameters
    assert list(q)[1:] == ["C", "n_models", "with_ensemble", "considered_classes", "rater_names", "n_candidates", "rounds"]
    assert q["with_ensemble"].default is True and q["n_candidates"].default == 16 and q["rounds"].default == 4
    r = inspect.signature(solve_temperature).parameters
    assert list(r) == ["sum_fn", "R", "n_candidates", "rounds", "log2_range"] and r["log2_range"].default == (-4., 4.)


# ------------------------------------------------------------------------------------------------------------ the entry points
def test_entry_points_refuse_before_they_launch():
    """Every call here is refused on its arguments alone (made-up addresses are never dereferenced on the device: nothing is
    launched), so the statuses can be read without a GPU."""
    from dct_amd import _lib
    lib = _lib.load()
    BAD, UNSUPPORTED = -1, _lib.ERR_UNSUPPORTED      # DCT_ERR_BAD_ARG, DCT_ERR_UNSUPPORTED

    def entries_of(S, entries):
        entries = [0x10000 + 0x1000 * s for s in range(max(S, 1))] if entries is None else entries
        return (ctypes.c_void_p * len(entries))(*entries)

    def sums(S=2, C=4, B=2, ppi=100, K=16, gt=0x2000, betas=0x5000, out=0x3000, counted=0x4000, entries=None, logits="array", ens=1):
        return lib.dct_temperature_sums(entries_of(S, entries) if logits == "array" else None, S, gt, B, ppi, C, 0xFF, ens, betas, K, out,
                                        counted, None)

    def apply(S=2, C=4, B=2, ppi=100, entries=None, outs=None, logits="array", out="array", beta="array", ens=1):
        R = max(S, 1) + (1 if ens == 1 else 0)
        outs = [0x20000 + 0x1000 * r for r in range(R)] if outs is None else outs
        return lib.dct_temperature_apply(entries_of(S, entries) if logits == "array" else None, S, B, ppi, C,
                                         (ctypes.c_float * 9)(*([1.0] * 9)) if beta == "array" else None, ens,
                                         (ctypes.c_void_p * len(outs))(*outs) if out == "array" else None, None)

    shared_bad = (dict(logits=None), dict(S=0), dict(S=-1), dict(B=0), dict(ppi=0), dict(entries=[0x10000, 0]), dict(ens=2), dict(ens=-1),
                  dict(C=4, entries=[0x10000, 0x11008]), dict(C=2, entries=[0x10000, 0x11004]), dict(C=3, entries=[0x10000, 0x11002]))
    shared_unsupported = (dict(S=9, entries=[0x10000] * 9), dict(C=0), dict(C=9), dict(B=65536), dict(ppi=1 << 31))
    for kw in shared_bad + (dict(gt=0), dict(betas=0), dict(out=0), dict(counted=0), dict(gt=0x2004), dict(out=0x3004), dict(counted=0x4004),
                            dict(betas=0x5002)):
        assert sums(**kw) == BAD, kw
    for kw in shared_unsupported + (dict(K=0), dict(K=17), dict(K=-1)):
        assert sums(**kw) == UNSUPPORTED, kw
    for kw in shared_bad + (dict(beta=None), dict(out=None), dict(outs=[0x20000, 0, 0x22000]), dict(outs=[0x20000, 0x21000, 0x22008]),
                            dict(C=2, outs=[0x20000, 0x21000, 0x22004]), dict(C=3, outs=[0x20000, 0x21002, 0x22000])):
        assert apply(**kw) == BAD, kw
    for kw in shared_unsupported:
        assert apply(**kw) == UNSUPPORTED, kw
