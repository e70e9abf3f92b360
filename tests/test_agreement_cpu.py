"""The rule of ``dct_confusion_counts`` (include/dct.h) as numpy references, checked against each other and, where scikit-learn is
installed, against ``confusion_matrix`` / ``cohen_kappa_score``: pairwise confusion matrices from the argmax (first maximum) of S
logit tensors and gt, Cohen's kappa and IoU in float64 from such a matrix.  test_agreement_gpu.py holds the device to these
references with ``==``.

kappa is compared at 1e-12 absolute: both sides are float64 over identical integers and differ only by the order of their sums
(|kappa| <= 1, a handful of roundings of 1.1e-16 each)."""
import numpy as np
import pytest
import torch


# ------------------------------------------------------------------------------------------------------------- references
def pair_list(R):
    return [(i, j) for i in range(R) for j in range(i + 1, R)]


def reference_counts(logits_list, gt, C):
    """logits_list: S arrays [B, ..., C]; gt: integer array [B, ...] or None -> int64 [B, P, C, C].  Rater s says argmax (first
    maximum) of logits_list[s]; gt is the last rater; a pixel whose gt is outside [0, C) is in no pair that contains gt."""
    B = logits_list[0].shape[0]
    raters = [np.asarray(l).reshape(B, -1, C).argmax(-1) for l in logits_list]       # np.argmax: the first maximum
    valid = [np.ones_like(raters[0], dtype=bool) for _ in raters]
    if gt is not None:
        g = np.asarray(gt).reshape(B, -1).astype(np.int64)
        ok = (g >= 0) & (g < C)
        raters.append(np.where(ok, g, 0))
        valid.append(ok)
    pairs = pair_list(len(raters))
    out = np.zeros((B, len(pairs), C, C), np.int64)
    for b in range(B):
        for p, (i, j) in enumerate(pairs):
            m = valid[i][b] & valid[j][b]
            out[b, p] = np.bincount(raters[i][b][m] * C + raters[j][b][m], minlength=C * C).reshape(C, C)
    return out


def kappa_from_matrix(M, cols=None):
    """Cohen's kappa, unweighted, float64; ``cols``: zero every other column first (the pixels whose second rater is in cols)."""
    M = np.array(M, dtype=np.float64)
    if cols is not None:
        drop = [c for c in range(M.shape[1]) if c not in cols]
        M[:, drop] = 0.0
    n = M.sum()
    if n == 0:
        return np.nan
    po = np.trace(M) / n
    pe = float(M.sum(1) @ M.sum(0)) / (n * n)
    if pe == 1.0:
        return np.nan
    return (po - pe) / (1.0 - pe)


def iou_from_matrix(M):
    M = np.array(M, dtype=np.float64)
    d = np.diag(M)
    den = M.sum(1) + M.sum(0) - d
    return np.array([d[c] / den[c] if den[c] else np.nan for c in range(len(d))])


def onehot(cls, C):
    return (np.asarray(cls)[..., None] == np.arange(C)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ tests
def test_pair_index_formula():
    from dct_amd.metrics import pair_index
    for R in range(2, 10):
        pairs = pair_list(R)
        assert len(pairs) == R * (R - 1) // 2
        for p, (i, j) in enumerate(pairs):
            assert i * (2 * R - i - 1) // 2 + (j - i - 1) == p
            assert pair_index(i, j, R) == p


def test_reference_counts_on_a_hand_built_case():
    C = 3
    a = np.array([[0, 0, 1, 2, 2, 1]])
    b = np.array([[0, 1, 1, 2, 0, 1]])
    g = np.array([[0, 0, 1, 255, -1, 3]])
    cnt = reference_counts([onehot(a, C), onehot(b, C)], g, C)
    assert cnt.shape == (1, 3, C, C)
    assert cnt[0, 0].tolist() == [[1, 1, 0], [0, 2, 0], [1, 0, 1]]          # a against b: all six pixels
    assert cnt[0, 1].tolist() == [[2, 0, 0], [0, 1, 0], [0, 0, 0]]          # a against gt: the three pixels with a valid gt
    assert cnt[0, 2].tolist() == [[1, 0, 0], [1, 1, 0], [0, 0, 0]]
    assert reference_counts([onehot(a, C), onehot(b, C)], None, C).shape == (1, 1, C, C)
    # exact ties go to the first class
    tie = np.zeros((1, 4, C), np.float32)
    tie[0, 1, 1] = tie[0, 1, 2] = 1.0
    assert reference_counts([tie, tie], None, C)[0, 0].tolist() == [[3, 0, 0], [0, 1, 0], [0, 0, 0]]


def test_kappa_and_iou_known_values():
    assert kappa_from_matrix([[20, 5], [10, 15]]) == pytest.approx(0.4, abs=1e-15)       # the textbook 2 x 2 example
    assert kappa_from_matrix(np.eye(3) * 7) == 1.0
    assert np.isnan(kappa_from_matrix(np.zeros((3, 3))))                                 # n = 0
    assert np.isnan(kappa_from_matrix([[9, 0], [0, 0]]))                                 # both constant: pe = 1
    assert kappa_from_matrix([[5, 5], [0, 0]]) == 0.0                                    # one constant rater: po = pe
    iou = iou_from_matrix([[3, 1, 0], [2, 4, 0], [0, 0, 0]])
    assert iou[0] == 3 / 6 and iou[1] == 4 / 7 and np.isnan(iou[2])


def test_meter_helpers_agree_with_the_references():
    from dct_amd.metrics import iou_of, kappa_of
    rng = np.random.default_rng(0)
    for C in (2, 3, 4, 8):
        M = rng.integers(0, 50, (5, 3, C, C))
        M[0, 0] = 0
        M[1, 1] = 0
        M[1, 1, 0, 0] = 11
        M[2, 2, :, 1:] = 0                                                              # with cols = [1, ...]: nothing left
        for cols in (None, list(range(1, C))):
            got = kappa_of(M, cols)
            ref = np.array([[kappa_from_matrix(M[r, p], cols) for p in range(3)] for r in range(5)])
            assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref).sum() >= 2
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12, equal_nan=True)
        ref = np.array([[iou_from_matrix(M[r, p]) for p in range(3)] for r in range(5)])
        np.testing.assert_allclose(iou_of(M), ref, rtol=1e-15, equal_nan=True)


@pytest.mark.parametrize("C", [2, 3, 4, 8])
def test_references_against_scikit_learn(C):
    sk = pytest.importorskip("sklearn.metrics")
    import warnings
    rng = np.random.default_rng(100 + C)
    n = 500
    cases = [(rng.integers(0, C, n), rng.integers(0, C, n)) for _ in range(6)]
    a = rng.integers(0, C, n)
    cases.append((a, np.where(rng.random(n) < 0.8, a, rng.integers(0, C, n))))         # mostly agreeing
    cases.append((np.full(n, C - 1), np.full(n, C - 1)))                                # both constant: NaN on both sides
    cases.append((np.full(n, 0), rng.integers(0, C, n)))                                # one constant: 0
    cases.append((rng.integers(0, C, n), np.full(n, 1)))
    seen_nan = 0
    for a, b in cases:
        M = reference_counts([onehot(a[None], C)], b[None], C)[0, 0]
        assert np.array_equal(M, sk.confusion_matrix(a, b, labels=list(range(C))))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = sk.cohen_kappa_score(a, b)
        got = kappa_from_matrix(M)
        assert np.isnan(got) == np.isnan(ref)
        seen_nan += int(np.isnan(ref))
        if not np.isnan(ref):
            assert abs(got - ref) <= 1e-12
        # the column mask against masking the pixels (the reference's considered_classes on the target, here b)
        cols = list(range(1, C))
        keep = np.isin(b, cols)
        got = kappa_from_matrix(M, cols)
        if keep.sum() == 0:
            assert np.isnan(got)
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = sk.cohen_kappa_score(a[keep], b[keep])
        assert np.isnan(got) == np.isnan(ref)
        if not np.isnan(ref):
            assert abs(got - ref) <= 1e-12
    assert seen_nan >= 1


def test_meter_refuses_cpu_tensors_and_wrong_lists():
    from dct_amd.metrics import AgreementMeter
    m = AgreementMeter(method='2d', C=3, n_models=2, with_gt=True)
    assert m.pairs == ["S0_S1", "S0_gt", "S1_gt"]
    assert AgreementMeter(C=3, n_models=3, with_gt=False).pairs == ["S0_S1", "S0_S2", "S1_S2"]
    assert AgreementMeter(C=3, n_models=2, rater_names=["S0", "ensemble"]).pairs == ["S0_ensemble", "S0_gt", "ensemble_gt"]
    p = torch.zeros(2, 3, 4, 5)
    g = torch.zeros(2, 1, 4, 5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.add([p, p], g)
    with pytest.raises(RuntimeError):
        m.add([p], g)
    with pytest.raises(RuntimeError):
        m.add([p, p, p], g)
    # nothing added: empty statistics, no device needed
    mean, std, n = m.kappa()
    assert n.tolist() == [0, 0, 0] and bool(torch.isnan(mean).all()) and bool(torch.isnan(std).all())
    assert m.confusion().shape == (3, 3, 3) and int(m.confusion().sum()) == 0
    assert np.isnan(m.summary()["mKappa"])
