"""The VAT launches of csrc/vat.hip (``K.vat_noise``, ``K.vat_sumsq``, ``K.vat_perturb``) and ``VATGenerator`` against the float64
reference of tests/vat_ref.py.

Sizes: per in {1, 3, 255, 256, 257, 4*37*41 + 1, 65536} x N in {1, 3, 16} -- one element, an odd ``per`` (every second sample off the
16-byte alignment: the scalar walk), both sides of a block's 256 threads, a tail behind the vector groups, two blocks per sample with an
odd chunk boundary, and 16 blocks per sample.

Bounds.
  norms      rtol 1e-12 x the number of addends (float64 sums in another order).
  x_out, r   8 x 2^-24 x (|x| + |r|) per element: the fp32 rounding of the scale (relative 2^-24, carried by r), of the product and of the
             sum, 4 ulp derived, twice that asserted (the worst CPU emulation reached 0.18 of the bound).
  noise      1e-5 absolute: rho <= sqrt(-2 log 2^-24) = 5.77 times the error of the fp32 angle 2 pi u2 (2 pi 2^-24 at most) plus the
             rounding of rho and of the product (numpy fp32 against fp64 gave 1.6e-6).  A wrong Philox word moves a value by O(1), so
             this pins the 24 bits of every word the rule uses; the second word of each pair is also recovered from the angle.
  generator  the device's largest deviation from the float64 reference is at most 4 x that of the same rule in fp32 torch on the CPU
             (another summation order, not another algorithm) plus the per-element floor above.
"""
import math

import numpy as np
import pytest
import torch

import vat_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
PERS = [1, 3, 255, 256, 257, 4 * 37 * 41 + 1, 65536]
NS = [1, 3, 16]
SEED = 0x5DEECE66D + (0x2545F49 << 32)


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


def _data(N, per, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, per, generator=g, dtype=torch.float32)
    d = torch.randn(N, per, generator=g, dtype=torch.float32) * scale
    return x, d


def _check_perturb(K, x, d, radius, xd=None, dd=None):
    """One sumsq + perturb of (x, d) (CPU fp32 tensors; ``xd`` / ``dd``: their device copies when the caller placed them) against the
    float64 reference.  -> the largest error as a share of the bound."""
    xd = x.to(DEV) if xd is None else xd
    dd = d.to(DEV) if dd is None else dd
    ws = K.vat_sumsq(dd)
    xo, r, nrm = K.vat_perturb(xd, dd, radius, ws, want_norms=True)
    xo2, r2, nrm2 = K.vat_perturb(xd, dd, radius, K.vat_sumsq(dd), want_norms=True)
    assert torch.equal(xo, xo2) and torch.equal(r, r2) and torch.equal(nrm, nrm2)         # a second launch: the same bits
    x_ref, r_ref, n_ref = vat_ref.perturb(x, d, radius)
    per = x.shape[1]
    np.testing.assert_allclose(nrm.cpu().numpy(), n_ref.numpy(), rtol=1e-12 * per)
    bound = 8 * U * (x.double().abs() + r_ref.abs())
    ex, er = (xo.cpu().double() - x_ref).abs(), (r.cpu().double() - r_ref).abs()
    assert torch.all(ex <= bound) and torch.all(er <= bound), (float((ex / bound).max()), float((er / bound).max()))
    # without r_out: the same x_out
    assert torch.equal(K.vat_perturb(xd, dd, radius, ws, want_r=False)[0], xo)
    return max(float((ex / bound).max()), float((er / bound).max()))


@pytest.mark.parametrize("per", PERS)
def test_norms_and_perturbation_against_float64(K, per):
    worst = 0.0
    for N in NS:
        x, d = _data(N, per, 17 * N + per)
        for radius in (0.5, 10.0):
            worst = max(worst, _check_perturb(K, x, d, radius))
    print(f"per = {per}: largest error {worst:.3f} of the bound")


@pytest.mark.parametrize("per", [257, 4 * 37 * 41 + 1, 65536])
def test_buffers_off_the_vector_alignment_take_the_scalar_walk(K, per):
    """x, d and the outputs' alignment decide the walk, not only ``per``: tensors that start 4 bytes into an allocation."""
    N = 3
    x, d = _data(N, per, 5 + per)
    xd = torch.empty(N * per + 1, dtype=torch.float32, device=DEV)[1:].view(N, per).copy_(x)
    dd = torch.empty(N * per + 1, dtype=torch.float32, device=DEV)[1:].view(N, per).copy_(d)
    assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    _check_perturb(K, x, d, 2.0, xd, dd)
    # the partials do not depend on the walk's access width only through the order of the adds: both stay within the norm's bound, and the
    # aligned and the misaligned copy of one tensor give the same perturbation within the element bound (checked above against float64)


@pytest.mark.parametrize("per", [3, 257, 65536])
def test_samples_without_a_direction_come_back_unchanged(K, per):
    """A zero sample, an inf sample and a NaN sample: exactly x and exactly 0, whatever else is in the sample; their neighbours are not touched
    by it."""
    x, d = _data(5, per, 3 + per)
    d[0].zero_()
    d[1, per // 2] = float("inf")
    d[2, per - 1] = float("nan")
    d[3, 0] = float("-inf")
    xd, dd = x.to(DEV), d.to(DEV)
    ws = K.vat_sumsq(dd)
    xo, r, nrm = K.vat_perturb(xd, dd, 1.5, ws, want_norms=True)
    for n in range(4):
        assert torch.equal(xo[n], xd[n]) and torch.count_nonzero(r[n]) == 0 and not torch.isnan(r[n]).any()
    nrm = nrm.cpu()
    assert nrm[0] == 0 and math.isinf(nrm[1]) and math.isnan(nrm[2]) and math.isinf(nrm[3])
    x_ref, r_ref, _ = vat_ref.perturb(x[4:], d[4:], 1.5)
    bound = 8 * U * (x[4:].double().abs() + r_ref.abs())
    assert torch.all((xo[4:].cpu().double() - x_ref).abs() <= bound) and torch.all((r[4:].cpu().double() - r_ref).abs() <= bound)


@pytest.mark.parametrize("scale", [1e-20, 1e+20])
@pytest.mark.parametrize("per", [257, 65536])
def test_tiny_and_huge_directions_keep_their_direction(K, per, scale):
    """Squares of 1e-20 and of 1e+20 leave fp32's range but not float64's."""
    x, d = _data(3, per, 11 + per, scale)
    sq = float((d * d).max())                                                    # fp32 squares: below the smallest normal, or inf
    assert sq < 2.0 ** -126 or sq == float("inf")
    _check_perturb(K, x, d, 2.0)


# ------------------------------------------------------------------------------------------------ noise
def _recovered_angle_words(z):
    """float64 noise [.., 2] pairs -> (rho, the 24-bit integer of u2 the angle stands for)."""
    ev, od = z[..., 0], z[..., 1]
    k = np.mod(np.arctan2(od, ev) / (2 * np.pi), 1.0) * 2.0 ** 24
    return np.hypot(ev, od), k


@pytest.mark.parametrize("per", PERS)
def test_noise_against_the_philox_reference(K, per):
    for N in NS:
        call = 7 + N
        d = torch.full((N, per), float("nan"), dtype=torch.float32, device=DEV)
        _, ws = K.vat_noise(d, SEED, offset=call)
        ref = vat_ref.noise((N, per), SEED, call)
        got = d.cpu().double().numpy()
        err = np.abs(got - ref).max()
        assert err <= 1e-5, (N, per, err)
        # the partials the noise launch wrote are those of the tensor it wrote, bit for bit
        assert torch.equal(ws, K.vat_sumsq(d))
        np.testing.assert_allclose(K.vat_perturb(d, d, 1.0, ws, want_r=False, want_norms=True)[2].cpu().numpy(),
                                   np.sqrt((ref * ref).sum(1)), rtol=0, atol=1e-5 * math.sqrt(per))     # (the triangle inequality)
        # the same call again: the same bits; the device-counter form of the same call: the same bits, the counter untouched
        d2 = torch.empty_like(d)
        K.vat_noise(d2, SEED, offset=call)
        calls = torch.tensor([call - 1], dtype=torch.int64, device=DEV)
        d3 = torch.empty_like(d)
        K.vat_noise(d3, SEED, calls=calls)
        assert torch.equal(d, d2) and torch.equal(d, d3) and int(calls.item()) == call - 1
        # the second word of every pair, recovered from the angle: off by at most (1e-5 / rho) / (2 pi) 2^24 of 2^24 (circular)
        n2 = (N * per) // 2 * 2
        if n2:
            words = vat_ref.philox_words(4 * ((N * per + 3) // 4), SEED, call).reshape(-1, 2)[: n2 // 2, 1]
            k_ref = (words >> np.uint64(8)).astype(np.float64)
            rho, k = _recovered_angle_words(got.reshape(-1)[:n2].reshape(-1, 2))
            off = np.abs(k - k_ref)
            off = np.minimum(off, 2.0 ** 24 - off)
            sel = rho > 0.1
            assert np.all(off[sel] <= 1e-5 / rho[sel] / (2 * np.pi) * 2.0 ** 24 + 1)


def test_noise_moments_counter_and_successive_draws(K):
    N, per = 16, 65536
    n = N * per
    calls = torch.tensor([41], dtype=torch.int64, device=DEV)
    d1 = torch.empty(N, per, dtype=torch.float32, device=DEV)
    _, ws = K.vat_noise(d1, SEED, calls=calls)
    assert int(calls.item()) == 41                                              # the noise launch only reads the word
    x = torch.zeros_like(d1)
    xo, _, _ = K.vat_perturb(x, d1, 1.0, ws, want_r=False, calls_advance=calls)
    assert int(calls.item()) == 42                                              # the perturb launch given the pointer: exactly one on
    K.vat_perturb(x, d1, 1.0, ws, want_r=False)
    assert int(calls.item()) == 42                                              # ... and not without it
    d2 = torch.empty_like(d1)
    K.vat_noise(d2, SEED, calls=calls)
    assert not torch.equal(d1, d2) and float((d1 == d2).double().mean()) < 1e-3  # two successive draws differ
    ref = torch.empty_like(d1)
    K.vat_noise(ref, SEED, offset=43)
    assert torch.equal(d2, ref)
    z = d1.double()
    mean, var = float(z.mean()), float(z.var())
    print(f"device noise over 2^20 elements: |mean| {abs(mean):.2e} (limit {5 / math.sqrt(n):.2e}), |var - 1| {abs(var - 1):.2e} "
          f"(limit {5 * math.sqrt(2 / n):.2e})")
    assert abs(mean) < 5 / math.sqrt(n) and abs(var - 1) < 5 * math.sqrt(2 / n)
    # x = 0, radius 1: every sample of x_out has norm 1
    np.testing.assert_allclose(vat_ref.norms(xo.cpu()).numpy(), 1.0, rtol=1e-6)


def test_bad_arguments_are_refused(K):
    d = torch.zeros(2, 8, dtype=torch.float32, device=DEV)
    ws = K.vat_sumsq(d)
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="dct_vat_perturb"):
            K.vat_perturb(d, d, radius, ws)
    with pytest.raises(RuntimeError, match="workspace"):
        K.vat_sumsq(d, ws[:1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.vat_sumsq(torch.zeros(2, 8))


# ------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize("ip", [1, 2])
def test_generator_on_a_toy_module_against_float64(K, ip):
    """VATGenerator over a module with no convolution library behind it, explicit direction, xi = 0.01, eps = 0.5.  Figures as printed on
    an MI355X: profiles/vat.txt."""
    from dct_amd.utils.AEGenerator import VATGenerator
    xi, eps = 0.01, 0.5
    net64 = vat_ref.ToyNet()
    net32 = vat_ref.ToyNet(dtype=torch.float32)
    net_dev = vat_ref.ToyNet(dtype=torch.float32).to(DEV)
    gen = VATGenerator(net_dev, xi=xi, eplision=eps, ip=ip)
    for seed in range(4):
        x, d0 = vat_ref.toy_case(seed)
        x32, d32 = x.float(), d0.float()
        x_ref, r_ref, p_ref = vat_ref.generate(net64, x32.double(), d32.double(), xi, eps, ip)
        _, r_cpu, _ = vat_ref.generate(net32, x32, d32, xi, eps, ip)
        with torch.no_grad():
            l = net64(x32.double())
            kl_rand = vat_ref.kl_per_sample(l, net64(vat_ref.perturb(x32.double(), d32.double(), eps)[0]))
            ratio_ref = vat_ref.kl_per_sample(l, net64(x_ref)) / kl_rand
        assert torch.all(ratio_ref > 1.5), ratio_ref                            # the property, on the reference first
        x_adv, r, probs = gen(x32.to(DEV), direction=d32.to(DEV))
        assert gen.noise._calls == 0 and gen.noise._seed is None                 # an explicit direction draws nothing
        assert all(p.requires_grad and p.grad is None for p in net_dev.parameters())
        r_dev, x_dev = r.cpu().double(), x_adv.cpu().double()
        cpu_dev = float((r_cpu.double() - r_ref).abs().max())
        dev_dev = float((r_dev - r_ref).abs().max())
        floor = 8 * U * (x32.double().abs() + r_ref.abs())
        print(f"ip = {ip}, seed {seed}: largest |r - float64| on the device {dev_dev:.3e}, in fp32 torch on the CPU {cpu_dev:.3e}")
        assert torch.all((r_dev - r_ref).abs() <= 4 * cpu_dev + floor)
        assert torch.all((x_dev - (x32.double() + r_dev)).abs() <= 2 * U * x_dev.abs())
        np.testing.assert_allclose(vat_ref.norms(r_dev).numpy(), eps, rtol=1e-5)
        np.testing.assert_allclose(probs.cpu().double().numpy(), p_ref.numpy(), atol=1e-6)
        with torch.no_grad():
            ratio = vat_ref.kl_per_sample(l, net64(x_dev)) / kl_rand
        assert torch.all(ratio > 1.5), ratio                                     # ... then on the device


def test_generator_draws_its_own_noise_and_advances_the_counter(K):
    from dct_amd.utils.AEGenerator import VATGenerator, VATNoise
    net = vat_ref.ToyNet(dtype=torch.float32).to(DEV)
    x = vat_ref.toy_case(0)[0].float().to(DEV)
    noise = VATNoise(seed=SEED)
    gen = VATGenerator(net, xi=0.01, eplision=0.5, ip=2, noise=noise)
    a = gen(x, None, None)
    assert noise._calls == 1 and int(noise.state(DEV).item()) == 1
    b = gen(x)
    assert noise._calls == 2 and int(noise.state(DEV).item()) == 2
    assert not torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    np.testing.assert_allclose(vat_ref.norms(b[1].cpu()).numpy(), 0.5, rtol=1e-5)
    # the same seed from the start: the same two results
    gen2 = VATGenerator(net, xi=0.01, eplision=0.5, ip=2, noise=VATNoise(seed=SEED))
    a2, b2 = gen2(x), gen2(x)
    assert torch.equal(a[0], a2[0]) and torch.equal(b[1], b2[1])
    # ... and the first is the generator run from draw number 1 as a caller-supplied direction
    d0 = torch.empty_like(x)
    K.vat_noise(d0, SEED, offset=1)
    c = VATGenerator(net, xi=0.01, eplision=0.5, ip=2)(x, direction=d0)
    assert torch.equal(c[0], a[0]) and torch.equal(c[1], a[1])
