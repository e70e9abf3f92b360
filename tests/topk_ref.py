"""The top-k cross entropy of include/dct.h (``dct_topk_ce_*``) in float64 plain torch, for tests/test_topk_ce_cpu.py and
tests/test_topk_ce_gpu.py:

  * ``k_of``: K = min(N, max(1, int(N k / 100))), Python's arithmetic (IEEE double, the order of the header);
  * ``Ref``: the map v = w l (tests/focal_ref.py's ``Ref`` at gamma = 0, from exactly the fp32 logits and weights the kernels see), K, tau,
    the value and its autograd gradient through ``torch.topk``, and the per-pixel map bound e (``focal_ref.ce_bounds``);
  * ``selection``: (K, N, tau, n_gt, n_eq, a) of ANY stored map under the header's tie rule -- a_i = 1 above tau, (K - n_gt) / n_eq on
    it, 0 below and on uncounted pixels --, which the GPU tests apply to the device's own map;
  * ``inputs``: tests/focal_ref.py's tensors (a quarter ignored, stray targets, sentinels at the seams of both grids, the non-dyadic
    weight set with its zero weight) with one of three plants:
      ``tie``      m counted pixels get identical logits and one target (the class of the largest weight, target logit 50 below the
                   rest), with m = 2 (K - n_above): the K-th largest falls strictly inside the group;
      ``cluster``  C = 2, weight = NULL: 300 pixels with target logit -D_j against 0, D_j = 1000 + j ulp(1000), so v_j = D_j exactly in
                   fp32 and the keys differ in the last pass's digits only; ``k_for`` then puts tau inside the cluster;
      ``same``     every pixel identical and counted: n_gt = 0, a_i = K / N;
    the zero-weight class of the weight set is a mass tie at v = 0 by itself (k = 100 makes it straddle K)."""
import math

import torch

import focal_ref as F

U, SUM_DEPTH, IGN = F.U, F.SUM_DEPTH, F.IGN
ULP_1000 = 2.0 ** -14           # the spacing of fp32 in [512, 1024)
CLUSTER = 300


def k_of(N, k):
    return min(N, max(1, int(N * k / 100))) if N else 0


def k_for(N, K):
    """A k_percent under which k_of(N, k) == K (checked)."""
    k = min(100.0, 100.0 * (K + 0.5) / N)
    assert k_of(N, k) == K and 0 < k <= 100, (N, K, k)
    return k


def selection(v, keep, k):
    """The header's selection on a stored map ``v`` ([P], any float dtype) with counted mask ``keep``: (K, N, tau, n_gt, n_eq, a [P]
    float64).  Comparisons are the dtype's own (-0 == +0)."""
    vc = v[keep]
    N = int(vc.numel())
    K = k_of(N, k)
    a = torch.zeros(v.shape[0], dtype=torch.float64)
    if N == 0:
        return 0, 0, None, 0, 0, a
    tau = torch.kthvalue(vc, N - K + 1).values            # the K-th largest
    gt, eq = keep & (v > tau), keep & (v == tau)
    n_gt, n_eq = int(gt.sum()), int(eq.sum())
    assert n_gt < K <= n_gt + n_eq
    a[gt] = 1.0
    a[eq] = (K - n_gt) / n_eq
    return K, N, tau, n_gt, n_eq, a


def inputs(P, C, w, stray, seed, plant=None, k=10.0):
    """-> (generator, x, t, t_ref, sentinels, planted indices or None).  ``w``: the fp32 weights the map is formed with (ones for NULL)."""
    if plant == "same":
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(1, C, generator=g).repeat(P, 1).contiguous()
        t = torch.full((P,), int(torch.nonzero(w)[0, 0]), dtype=torch.int64)
        return g, x, t, t.clone(), F.sentinels(P), torch.arange(P)
    g, x, t, t_ref, sen, plants = F.inputs(P, C, w, stray, seed)
    if plant is None:
        return g, x, t, t_ref, sen, None
    special = set(sen.tolist()) | {int(i) for p in plants.values() for i in p.tolist()}
    if plant == "cluster":
        assert C == 2 and not stray and P > 1000 + 7 * CLUSTER
        idx = 1000 + 7 * torch.arange(CLUSTER)
        assert not special & set(idx.tolist())
        D = 1000.0 + torch.arange(CLUSTER, dtype=torch.float64) * ULP_1000
        assert torch.equal(D.float().double(), D)         # every D_j is an fp32 number
        t[idx] = 0
        t_ref[idx] = 0
        x[idx, 0] = -D.float()
        x[idx, 1] = 0.0
        return g, x, t, t_ref, sen, idx
    assert plant == "tie"
    keep = t_ref != IGN
    v = F.Ref(x, t_ref, w, C, 0.0).f
    K = k_of(int(keep.sum()), k)
    c = int(torch.argmax(w))
    row = torch.zeros(C)
    row[c] = -50.0
    v0 = float(w[c]) * (50.0 + math.log(C - 1))
    free = [i for i in torch.nonzero(keep)[:, 0].tolist() if i not in special]
    # the group replaces counted pixels below v0 (N and the pixels above it stay), taken from the front and the back of the walk
    below = [i for i in free if v[i].item() < v0]
    n_above = int((keep & (v > v0)).sum())
    m = 2 * (K - n_above)
    assert 2 <= m <= len(below), (K, n_above, len(below))
    idx = torch.tensor(sorted(below[:m // 2] + below[-(m - m // 2):]))
    x[idx] = row
    t[idx] = c
    t_ref[idx] = c
    return g, x, t, t_ref, sen, idx


class Ref:
    """float64 reference of one (x, t, w, k): the map (with a graph), K, N, tau, the value, and the map's per-pixel bound."""

    def __init__(self, x, t_ref, w, C, k):
        self.r = r = F.Ref(x, t_ref, w, C, 0.0)
        self.keep, self.v = r.keep, r.f
        self.N = int(r.keep.sum())
        self.K = k_of(self.N, k)
        _, self.e, self.grad_bound = F.ce_bounds(r)
        if self.N == 0:
            self.value, self.tau = None, None
            return
        idx = torch.nonzero(r.keep)[:, 0]
        top = torch.topk(r.fmap[idx], self.K)
        self.value = top.values.mean()                      # (with a graph)
        self.tau = top.values[-1].item()
        self.top_abs = top.values.detach().abs().sum().item()

    def sum_tol(self, sum_abs, K):
        """The fp32 sum of the entries above tau along a tree of SUM_DEPTH levels, divided by K."""
        return SUM_DEPTH * U * sum_abs / K

    def bracket(self):
        """(the K-th largest of v - e, of v + e, the top-k mean of v - e, of v + e) over the counted pixels: the top-k mean and every
        order statistic are monotone in each entry, so any map within e of v has its tau and its value between these."""
        lo, hi = (self.v - self.e)[self.keep], (self.v + self.e)[self.keep]
        tl, th = torch.topk(lo, self.K).values, torch.topk(hi, self.K).values
        return tl[-1].item(), th[-1].item(), tl.mean().item(), th.mean().item()

    def grad(self, gfac, old=None):
        """gfac * d value / d x (+ old) by autograd through torch.topk."""
        (d,) = torch.autograd.grad(self.value * gfac, self.r.xd, retain_graph=True)
        return d if old is None else d + old.double()
