"""The VAT rule of include/dct.h in numpy / torch float64: the reference of tests/test_vat_cpu.py, tests/test_vat_gpu.py.

noise       flat element e takes word e & 3 of philox4x32_10(seed, (call << 40) + (e >> 2)); words (r0, r1) and (r2, r3) give two normals each
            by Box-Muller with u1 = ((ra >> 8) + 1) 2^-24, u2 = (rb >> 8) 2^-24: rho cos(2 pi u2) on the even element, rho sin(2 pi u2) on the odd.
norms       the L2 norm of every sample in float64.
perturb     x + (radius / norm) d per sample; a sample whose norm is 0 or not finite comes back unchanged, r = 0.
generate    the whole generator over a callable net, in the dtype of its input.
"""
import math

import numpy as np
import torch

from test_pointwise_kernels_scale_gpu import philox4x32_10

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox_words(n, seed, call):
    """uint64 [n] holding the 32-bit word every flat element 0 .. n - 1 takes."""
    G = (n + 3) // 4
    with np.errstate(over="ignore"):
        ctr = np.uint64((call << 40) & (2 ** 64 - 1)) + np.arange(G, dtype=np.uint64)
    zero = np.zeros(G, dtype=np.uint64)
    r = philox4x32_10((np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)), (ctr & _M32, ctr >> _S32, zero, zero))
    return np.stack(r, axis=-1).reshape(-1)[:n]


def noise(shape, seed, call):
    """float64 numpy array of ``shape``: the noise of rule 2, every function in double."""
    n = int(np.prod(shape))
    w = philox_words(4 * ((n + 3) // 4), seed, call).reshape(-1, 2, 2)          # [group, pair, (ra, rb)]
    u1 = ((w[..., 0] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (w[..., 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    rho = np.sqrt(-2.0 * np.log(u1))
    out = np.stack((rho * np.cos(2.0 * np.pi * u2), rho * np.sin(2.0 * np.pi * u2)), axis=-1)
    return out.reshape(-1)[:n].reshape(shape)


def norms(d):
    """float64 [N]: the L2 norm of every sample of the torch tensor ``d`` ([N, ...]), squares and sum in float64."""
    dd = d.detach().double().reshape(d.shape[0], -1)
    return (dd * dd).sum(1).sqrt()


def perturb(x, d, radius, dtype=torch.float64):
    """-> (x_out, r, norms).  ``dtype`` float64: the reference; float32: the rule with the kernel's roundings (scale, product, sum)."""
    nrm = norms(d)
    ok = torch.isfinite(nrm) & (nrm > 0)
    scale = torch.where(ok, radius / torch.where(ok, nrm, torch.ones_like(nrm)), torch.zeros_like(nrm)).to(dtype)
    shape = (-1,) + (1,) * (d.dim() - 1)
    okb = ok.reshape(shape)
    r = torch.where(okb, scale.reshape(shape) * torch.where(okb, d.to(dtype), torch.zeros((), dtype=dtype)), torch.zeros((), dtype=dtype))
    return x.to(dtype) + r, r, nrm


def kl_mean(l_clean, l_hat):
    """The mean over pixels of KL(softmax(l_clean) || softmax(l_hat)), logits [N, C, H, W] (dct_kl_logits_fwd without its 1e-10)."""
    y = torch.softmax(l_clean, 1)
    return (y * (torch.log_softmax(l_clean, 1) - torch.log_softmax(l_hat, 1))).sum(1).mean()


def kl_per_sample(l_clean, l_hat):
    y = torch.softmax(l_clean, 1)
    return (y * (torch.log_softmax(l_clean, 1) - torch.log_softmax(l_hat, 1))).sum(1).flatten(1).mean(1)


def generate(net, x, direction, xi, eps, ip):
    """The generator of the rule over ``net`` (a callable: [N, Cin, H, W] -> logits [N, C, H, W]) in x's dtype.
    -> (x_adv, r, softmax(l)); the gradient through autograd."""
    dt = x.dtype
    with torch.no_grad():
        l = net(x)
    d = direction.to(dt)
    for _ in range(ip):
        xp = perturb(x, d, xi, dt)[0].detach().requires_grad_(True)
        D = kl_mean(l, net(xp))
        (d,) = torch.autograd.grad(D, xp)
    x_adv, r, _ = perturb(x, d, eps, dt)
    return x_adv.detach(), r.detach(), torch.softmax(l, 1)


class ToyNet(torch.nn.Module):
    """A network with no convolution library behind it: einsum(W, tanh(2x - 1)) + 0.5 einsum(V, roll(x, 1, 3) * roll(x, 1, 2)), W and V
    seeded [4, 3] matrices."""

    def __init__(self, seed=0, dtype=torch.float64):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.W = torch.nn.Parameter(torch.randn(4, 3, generator=g, dtype=torch.float64).to(dtype))
        self.V = torch.nn.Parameter(torch.randn(4, 3, generator=g, dtype=torch.float64).to(dtype))

    def forward(self, x):
        return (torch.einsum("kc,nchw->nkhw", self.W, torch.tanh(2 * x - 1)) +
                0.5 * torch.einsum("kc,nchw->nkhw", self.V, torch.roll(x, 1, 3) * torch.roll(x, 1, 2)))


def toy_case(seed):
    """-> (x, d0): a seeded float64 batch [3, 3, 5, 7] in [0, 1] and a seeded direction."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.rand(3, 3, 5, 7, generator=g, dtype=torch.float64)
    d0 = torch.randn(3, 3, 5, 7, generator=g, dtype=torch.float64)
    return x, d0


SQRT_PER = math.sqrt(3 * 5 * 7)
