"""FGSM adversarial-example generator with the reference's interface
(/root/reference/generalframework/utils/AEGenerator.py:9-51).

``FSGMGenerator(net, eplision)(img, gt, criterion) -> (adv_img, noise, softmax(pred))``.
Differences that are not observable by the caller:
  * the backward to the input skips the weight-gradient GEMMs (the reference computes them and
    then ``net.zero_grad()``s them away, :27-30) -- parameters are frozen for the duration;
  * ``x + eps*sign(g)`` is one HIP kernel (K11), the pseudo-label argmax another (K10).

``VATGenerator`` (the reference's :54-119, broken as written there; the rule is restated in include/dct.h, "VAT") is the label-free
generator with the same call contract; ``VATNoise`` holds its random start's seed and draw counter.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from .. import hip_ops as K
from ..loss.loss import softmax_channels, _pc


class FSGMGenerator(object):
    def __init__(self, net: nn.Module, eplision: float = 0.05) -> None:
        super().__init__()
        self.net = net
        self.eplision = eplision

    def __call__(self, img: Tensor, gt: Tensor, criterion: nn.Module) -> Tuple[Tensor, Tensor, Tensor]:
        assert img.shape.__len__() == 4
        assert img.shape[0] >= gt.shape[0]
        img.requires_grad = True
        if img.grad is not None:
            img.grad.zero_()
        self.net.zero_grad()
        params = [p for p in self.net.parameters() if p.requires_grad]
        for p in params:
            p.requires_grad_(False)
        try:
            pred = self.net(img)
            if img.shape[0] > gt.shape[0]:
                lp = _pc(pred.detach())
                pseudo = K.argmax(lp, lp.shape[3]).view(img.shape[0], 1, img.shape[2], img.shape[3])
                gt = torch.cat((gt, pseudo[gt.shape[0]:]), dim=0)
            loss = criterion(pred, gt.squeeze(1))
            (grad,) = torch.autograd.grad(loss, img, retain_graph=False)
        finally:
            for p in params:
                p.requires_grad_(True)
        adv_img, noise = self.adversarial_fgsm(img, grad, epsilon=self.eplision)
        self.net.zero_grad()
        return adv_img.detach(), noise.detach(), softmax_channels(pred.detach())

    @staticmethod
    def adversarial_fgsm(image: Tensor, data_grad: Tensor, epsilon: float = 0.01) -> Tuple[Tensor, Tensor]:
        """perturbed = image + epsilon*sign(grad); no clamp (AEGenerator.py:35-51)."""
        x = image.detach().to(torch.float32).contiguous()
        g = data_grad.detach().to(torch.float32).contiguous()
        xa, noise = K.fgsm_step(x, g, epsilon)
        return xa, noise


class VATNoise(object):
    """The random start of VATGenerator's search: a Philox seed, the draw counter as a 64-bit word on the device (``dct_vat_noise`` reads
    it, the perturb launch behind it advances it: a captured step draws fresh noise on every replay) and its host mirror ``_calls``.

    The seed comes from torch's global generator -- lazily, at the first draw, so that a trainer that stays on FGSM draws nothing new
    from it.  Under data parallelism the rank is mixed in (``mix_rank``: the same torch seed on every rank would give every rank the
    same noise), as ddp.FlatGradSync does for ``dropout_seed``."""

    def __init__(self, seed: Optional[int] = None) -> None:
        self._seed = None if seed is None else int(seed) & ((1 << 62) - 1)
        self._calls = 0                 # draws so far (the device word holds the same number in stream order)
        self._state: Optional[Tensor] = None
        self._rank_mixed = False

    @property
    def seed(self) -> int:
        if self._seed is None:
            self._seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        return self._seed

    def mix_rank(self, rank: int) -> None:
        if not self._rank_mixed:
            self._seed = (self.seed + 0x9E3779B97F4A7C15 * (rank + 1) * int(rank > 0)) & ((1 << 62) - 1)
            self._rank_mixed = True

    def state(self, device) -> Tensor:
        """The device word (int64[1]); created from the host mirror outside any capture."""
        device = torch.device(device)
        if self._state is None or self._state.device != device:
            self._state = torch.tensor([self._calls], dtype=torch.int64, device=device)
        return self._state

    def draw(self, like: Tensor) -> Tuple[Tensor, Tensor]:
        """-> (d, workspace): the next draw in the shape of ``like`` and its sum-of-squares partials.  The caller passes ``state(...)`` as
        ``calls_advance`` to the first K.vat_perturb behind this launch, then calls ``advanced()``."""
        d = torch.empty_like(like, dtype=torch.float32, memory_format=torch.contiguous_format)
        return K.vat_noise(d, self.seed, calls=self.state(like.device))

    def advanced(self) -> None:
        self._calls += 1


class VATGenerator(object):
    """Virtual adversarial examples (Miyato et al.; the rule: include/dct.h "VAT") with FSGMGenerator's call contract:

    ``VATGenerator(net, xi, eplision, ip, noise)(img, gt=None, criterion=None, direction=None) -> (adv_img, noise, softmax(pred))``.

    Label-free: ``gt`` and ``criterion`` are ignored.  From a random direction (``direction``, or else the next draw of ``noise``) it
    takes ``ip`` steps of power iteration towards the direction in which KL(softmax(net(img)) || softmax(net(img + xi * u))) grows
    fastest, and returns ``img + eplision * d / ||d||`` with the L2 norm taken per image; an image whose direction has norm 0 or a
    non-finite norm comes back unchanged.  Every forward pass is a training-mode pass of ``net`` as it stands (dropout draws a mask,
    BatchNorm updates its running statistics), as FSGMGenerator's is; parameters are frozen for the duration.  Any ``nn.Module`` works:
    the passes go through autograd; the noise, the norms and the scale-and-add are the HIP launches of csrc/vat.hip.

    ``eplision = 10`` is the reference's default (generalframework/utils/AEGenerator.py:56).  ``xi = 10`` is NOT its 1e-6: spread over
    an image that is below one fp32 ulp of a pixel in [0, 1] and invisible to a bf16 network; at 256 x 256, xi = 10 is 0.04 per pixel.
    Nobody has measured which values train best."""

    def __init__(self, net: nn.Module, xi: float = 10.0, eplision: float = 10.0, ip: int = 1, noise: Optional[VATNoise] = None) -> None:
        super().__init__()
        if not (xi > 0 and eplision > 0 and int(ip) == ip and ip >= 1):
            raise ValueError(f"dct_amd: VATGenerator needs xi > 0, eplision > 0 and a whole ip >= 1, got {xi!r}, {eplision!r}, {ip!r}")
        self.net = net
        self.xi, self.eplision, self.ip = float(xi), float(eplision), int(ip)
        self.noise = noise if noise is not None else VATNoise()

    def __call__(self, img: Tensor, gt: Optional[Tensor] = None, criterion: Optional[nn.Module] = None,
                 direction: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
        assert img.shape.__len__() == 4
        x = img.detach().to(torch.float32).contiguous()
        self.net.zero_grad()
        params = [p for p in self.net.parameters() if p.requires_grad]
        for p in params:
            p.requires_grad_(False)
        try:
            pred = self.net(x).detach()           # (nothing requires a gradient here: the pass records no graph)
            lp = _pc(pred)
            C_ = lp.shape[3]
            advance = None
            if direction is not None:
                d = direction.detach().to(torch.float32).contiguous()
                assert d.shape == x.shape
                ws = K.vat_sumsq(d)
            else:
                d, ws = self.noise.draw(x)
                advance = self.noise.state(x.device)
            for _ in range(self.ip):
                xp, _, _ = K.vat_perturb(x, d, self.xi, ws, want_r=False, calls_advance=advance)
                if advance is not None:
                    advance = None
                    self.noise.advanced()
                xp.requires_grad_(True)
                lph = _pc(self.net(xp))
                # the logit gradient of the mean KL (dct_kl_logits_bwd), handed to autograd for the pass back to the input
                dl = K.kl_logits_bwd(lph.detach().contiguous(), lp, C_, torch.empty_like(lph, memory_format=torch.contiguous_format))
                (g,) = torch.autograd.grad(lph, xp, grad_outputs=dl.view_as(lph), retain_graph=False)
                d = g.detach().to(torch.float32).contiguous()
                K.vat_sumsq(d, ws)
            adv_img, r, _ = K.vat_perturb(x, d, self.eplision, ws)
        finally:
            for p in params:
                p.requires_grad_(True)
        self.net.zero_grad()
        return adv_img.detach(), r.detach(), softmax_channels(pred.detach())
