"""The rule of ``dct_temperature_sums`` / ``dct_temperature_apply`` (include/dct.h) as a numpy reference, shared by
test_temperature_cpu.py and test_temperature_gpu.py.

Two precisions.  ``exact=False``: float64 throughout, from the fp32 logits and the candidates as they are given (the ensemble's
probabilities included); the sums it returns are what the device is compared with, as means.  ``exact=True``: every step of the rule in
fp32 in the rule's order (numpy's fp32 ``exp`` / ``log`` are not the device's, so this emulation is not compared with the device bit for
bit; it carries the properties that hold in any correctly rounded-or-not fp32 arithmetic, such as the exact scaling of (2 z, beta / 2))."""
import numpy as np

from test_calibration_cpu import rater_probs

UNIT = float(1 << 20)


def rater_logits(views, with_ensemble, exact):
    """views: S arrays [B, P, C] -> [R, B, P, C]: the views' logits and, last, u = log(p_ens + 1e-10) of the calibration rule's mean."""
    dt = np.float32 if exact else np.float64
    zs = [np.asarray(v, dtype=np.float32).astype(dt) for v in views]
    if with_ensemble:
        p = rater_probs(views, True, True, exact)[-1]
        zs.append(np.log((p + dt(1e-10)).astype(dt)).astype(dt))
    return np.stack(zs)


def counted_pixels(gt, B, P, C, classes=None):
    gt = np.asarray(gt).reshape(B, P).astype(np.int64)
    allowed = np.zeros(C, dtype=bool)
    allowed[list(range(C)) if classes is None else list(classes)] = True
    valid = (gt >= 0) & (gt < C)
    t = np.where(valid, gt, 0)
    return valid & allowed[t], t


def pixel_terms(z, t, beta, exact):
    """z [n, C] one rater's logits on n pixels of class t [n], one candidate -> (nll [n], g [n]) by the rule, in fp32 or float64."""
    dt = np.float32 if exact else np.float64
    z = z.astype(dt)
    x = (dt(beta) * z).astype(dt)
    m = x.max(-1)
    e = np.exp((x - m[:, None]).astype(dt)).astype(dt)
    s, ez = np.zeros(len(z), dtype=dt), np.zeros(len(z), dtype=dt)
    for c in range(z.shape[1]):                     # in class order
        s = (s + e[:, c]).astype(dt)
        ez = (ez + (e[:, c] * z[:, c]).astype(dt)).astype(dt)
    idx = np.arange(len(z))
    nll = (np.log(s).astype(dt) - (x[idx, t] - m).astype(dt)).astype(dt)
    g = ((ez / s).astype(dt) - z[idx, t]).astype(dt)
    return nll, g


def words(nll, g):
    """The integer words of the rule: rint(min(nll, 4095) 2^20), rint(clamp(g, +-2047) 2^20); a NaN contributes 0."""
    with np.errstate(invalid='ignore'):
        a = np.where(np.isnan(nll), 0.0, np.minimum(nll.astype(np.float64), 4095.0))
        b = np.where(np.isnan(g), 0.0, np.clip(g.astype(np.float64), -2047.0, 2047.0))
    return np.rint(a * UNIT).astype(np.int64), np.rint(b * UNIT).astype(np.int64)


def reference(views, gt, betas, classes=None, with_ensemble=False, exact=False):
    """views: S arrays [B, P, C]; betas [R, K] -> dict: sums int64 [R, K, 2] (the words of this precision, summed), nll / g float64
    [R, K] (the unrounded sums, NaN pixels as 0), N (counted pixels)."""
    z = rater_logits(views, with_ensemble, exact)
    R, B, P, C = z.shape
    betas = np.asarray(betas)
    assert betas.ndim == 2 and betas.shape[0] == R, (betas.shape, R)
    counted, t = counted_pixels(gt, B, P, C, classes)
    sel, ts = counted.reshape(-1), t.reshape(-1)[counted.reshape(-1)]
    K = betas.shape[1]
    sums, nll_s, g_s = np.zeros((R, K, 2), dtype=np.int64), np.zeros((R, K)), np.zeros((R, K))
    for r in range(R):
        zr = z[r].reshape(-1, C)[sel]
        for k in range(K):
            nll, g = pixel_terms(zr, ts, np.float32(betas[r, k]) if exact else betas[r, k], exact)
            wn, wg = words(nll, g)
            sums[r, k] = (wn.sum(), wg.sum())
            nll_s[r, k], g_s[r, k] = np.nan_to_num(nll.astype(np.float64), nan=0.0).sum(), np.nan_to_num(g.astype(np.float64), nan=0.0).sum()
    return dict(sums=sums, nll=nll_s, g=g_s, N=int(counted.sum()))


def sum_fn_of(views, gt, classes=None, with_ensemble=False, fp32_betas=False):
    """The ``sum_fn`` of ``metrics.solve_temperature`` on the float64 reference; ``fp32_betas``: the candidates rounded to fp32 first,
    as a device fit sees them."""
    def fn(betas):
        b = np.asarray(betas, dtype=np.float64)
        r = reference(views, gt, b.astype(np.float32).astype(np.float64) if fp32_betas else b, classes, with_ensemble)
        return r["sums"], r["N"]
    return fn


def applied(views, betas, with_ensemble=False):
    """float64 softmax(beta_r z_r) of every rater -> [R, B, P, C]."""
    z = rater_logits(views, with_ensemble, False)
    x = z * np.asarray(betas, dtype=np.float64).reshape(-1, 1, 1, 1)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def sampled_case(seed, N, C, scales, sigma=1.0):
    """Logits z0 ~ N(0, sigma), labels sampled from softmax(z0), the views a * z0 for a in ``scales`` (each calibrated at
    beta = 1 / a) -> (views: len(scales) fp32 arrays [1, N, C], gt [1, N])."""
    rng = np.random.default_rng(seed)
    z0 = rng.normal(0, sigma, (1, N, C))
    p = np.exp(z0 - z0.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    gt = (rng.random((1, N, 1)) > p.cumsum(-1)).sum(-1).clip(0, C - 1)
    return [(a * z0).astype(np.float32) for a in scales], gt
