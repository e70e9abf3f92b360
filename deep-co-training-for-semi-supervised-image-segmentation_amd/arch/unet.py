"""UNet of the reference (arch/network.py:115-130,153-171,196-240) as one HIP execution plan.

Same parameters, same ``state_dict`` keys and logical shapes as the reference module, but
the forward/backward are not a graph of ATen ops: ``forward`` runs a fixed sequence of
hand-written gfx950 kernels over NHWC activations (include/dct.h), and a single
``torch.autograd.Function`` node replays the matching backward sequence.

Data layout in HBM
  activations : NHWC, bf16 (default) or fp32 (parity mode); skip-concats are channel slices of
                one buffer (the producer writes its slice, nothing is copied);
  weights     : fp32 masters in one flat buffer, physically K-major ``[Cout][kh][kw][Cin]``
                (``[Cin][a][b][Cout]`` for ConvTranspose2d) exposed as strided views with the
                reference's logical shapes; per-step packs in the compute dtype for the forward
                and the data-gradient GEMMs;
  gradients   : weight/bias gradients are accumulated straight into the flat fp32 gradient
                buffer that ``p.grad`` views alias (see arch/flat.py).

No CPU path: inputs must be on the HIP device.
"""
from __future__ import annotations

import contextlib
import dataclasses
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from .. import hip_ops as K
from .flat import FlatParams
from .unet_route import BackwardFacts, ForwardFacts, ForwardRoute, plan_backward_pass, plan_forward_pass

_WIDTHS = (64, 128, 256, 512)


class _Slots(nn.Module):
    def __init__(self, layers: Dict[int, nn.Module]):
        super().__init__()
        for idx, layer in layers.items():
            self.add_module(str(idx), layer)

    def at(self, idx: int) -> nn.Module:
        return getattr(self, str(idx))


class _Holder(nn.Module):
    pass


class _ShapeOf:
    """Stands in the tape for an activation that is no longer stored: the backward plan sizes its gradient by it."""
    __slots__ = ("shape",)

    def __init__(self, t: torch.Tensor):
        self.shape = tuple(t.shape)


class _ConvP(nn.Module):
    """Parameters of nn.Conv2d(cin, cout, k): logical [cout,cin,k,k], physical [cout][k][k][cin]."""
    transposed = False

    def __init__(self, cin, cout, k):
        super().__init__()
        self.cin, self.cout, self.k = cin, cout, k
        self.weight = nn.Parameter(torch.empty(cout, k, k, cin).permute(0, 3, 1, 2))
        self.bias = nn.Parameter(torch.empty(cout))
        self.reset_parameters()

    def reset_parameters(self):
        # torch's nn.Conv2d default (kaiming_uniform a=sqrt(5)); the reference then applies
        # weights_init (arch/__init__.py:60-65) on top, as get_arch() does here.
        fan_in = self.weight.shape[1] * self.k * self.k
        bound = 1.0 / fan_in ** 0.5
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            self.bias.uniform_(-bound, bound)


class _ConvTP(_ConvP):
    """Parameters of nn.ConvTranspose2d(cin, cout, 2, stride=2): logical [cin,cout,2,2],
    physical [cin][a][b][cout]."""
    transposed = True

    def __init__(self, cin, cout):
        nn.Module.__init__(self)
        self.cin, self.cout, self.k = cin, cout, 2
        self.weight = nn.Parameter(torch.empty(cin, 2, 2, cout).permute(0, 3, 1, 2))
        self.bias = nn.Parameter(torch.empty(cout))
        self.reset_parameters()

    def reset_parameters(self):
        fan_in = self.weight.shape[1] * 4  # torch uses weight.size(1) * receptive field
        bound = 1.0 / fan_in ** 0.5
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            self.bias.uniform_(-bound, bound)


class _BNP(nn.Module):
    """nn.BatchNorm2d(c) parameters and buffers (eps 1e-5, momentum 0.1: torch defaults, as network.py:138,181 use)."""
    is_dct_batchnorm = True

    def __init__(self, c, eps=1e-5, momentum=0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = c, eps, momentum
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class UNet(nn.Module):
    """Drop-in for the reference ``UNet(in_channels=1, num_classes=2)`` (network.py:196) and, with ``batchnorm=True``
    (class ``UNet_bn`` below), for ``UNet_bn`` (network.py:243-290).

    ``compute_dtype``: torch.bfloat16 (MFMA bf16, fp32 accumulate) or torch.float32
    (v_mfma_f32_32x32x2_f32; the parity mode).  ``dropout_p`` is the p of the two
    ``nn.Dropout`` sites (network.py:165,210)."""

    batch_independent = True   # no BatchNorm: samples of a batch never interact

    def __init__(self, in_channels: int = 1, num_classes: int = 2, compute_dtype=torch.bfloat16,
                 dropout_p: float = 0.5, batchnorm: bool = False):
        super().__init__()
        self.batchnorm = bool(batchnorm)
        if self.batchnorm:
            self.batch_independent = False     # batch statistics couple the samples of a pass
        if in_channels != 1:
            raise ValueError("dct_amd UNet: the hot path is single-channel slices (in_channels=1)")
        if not 2 <= num_classes <= 8:
            raise ValueError("dct_amd UNet: 2 <= num_classes <= 8")
        if compute_dtype not in (torch.bfloat16, torch.float32):
            raise ValueError("dct_amd UNet: compute_dtype is torch.bfloat16 (MFMA bf16) or torch.float32; fp16 is an Enet mode")
        self.num_classes = num_classes
        self.compute_dtype = compute_dtype
        self.dropout_p = float(dropout_p)
        cin = in_channels
        bn = self.batchnorm
        # Sequential indices of the reference modules (they are the state_dict keys): UNetDec / UNetDec_bn (network.py:153-193),
        # centre (:204-212 / :251-261), UNetEnc / UNetEnc_bn (:115-150), enc1 (:216-221 / :265-271).  The plan addresses the
        # layers by role through self._roles: (first conv, its BatchNorm or None, second conv, its BatchNorm or None[, convT]).
        self._roles: Dict[str, tuple] = {}
        for lvl, width in enumerate(_WIDTHS, start=1):
            blk = _Holder()
            if bn:
                blk.down = _Slots({0: _ConvP(cin, width, 3), 1: _BNP(width), 3: _ConvP(width, width, 3)})
                self._roles[f"dec{lvl}"] = (blk.down.at(0), blk.down.at(1), blk.down.at(3), None)
            else:
                blk.down = _Slots({0: _ConvP(cin, width, 3), 2: _ConvP(width, width, 3)})
                self._roles[f"dec{lvl}"] = (blk.down.at(0), None, blk.down.at(2), None)
            setattr(self, f"dec{lvl}", blk)
            cin = width
        if bn:
            self.center = _Slots({0: _ConvP(512, 1024, 3), 1: _BNP(1024), 3: _ConvP(1024, 1024, 3), 4: _BNP(1024), 7: _ConvTP(1024, 512)})
            c = self.center
            self._roles["center"] = (c.at(0), c.at(1), c.at(3), c.at(4), c.at(7))
        else:
            self.center = _Slots({0: _ConvP(512, 1024, 3), 2: _ConvP(1024, 1024, 3), 5: _ConvTP(1024, 512)})
            c = self.center
            self._roles["center"] = (c.at(0), None, c.at(2), None, c.at(5))
        for lvl, (ci, feat, co) in {4: (1024, 512, 256), 3: (512, 256, 128), 2: (256, 128, 64)}.items():
            blk = _Holder()
            if bn:
                blk.up = _Slots({0: _ConvP(ci, feat, 3), 1: _BNP(feat), 3: _ConvP(feat, feat, 3), 4: _BNP(feat), 6: _ConvTP(feat, co)})
                u = blk.up
                self._roles[f"enc{lvl}"] = (u.at(0), u.at(1), u.at(3), u.at(4), u.at(6))
            else:
                blk.up = _Slots({0: _ConvP(ci, feat, 3), 2: _ConvP(feat, feat, 3), 4: _ConvTP(feat, co)})
                u = blk.up
                self._roles[f"enc{lvl}"] = (u.at(0), None, u.at(2), None, u.at(4))
            setattr(self, f"enc{lvl}", blk)
        if bn:
            self.enc1 = _Slots({0: _ConvP(128, 64, 3), 1: _BNP(64), 3: _ConvP(64, 64, 3)})
            self._roles["enc1"] = (self.enc1.at(0), self.enc1.at(1), self.enc1.at(3), None)
        else:
            self.enc1 = _Slots({0: _ConvP(128, 64, 3), 2: _ConvP(64, 64, 3)})
            self._roles["enc1"] = (self.enc1.at(0), None, self.enc1.at(2), None)
        self.final = _ConvP(64, num_classes, 1)

        self._convs: List[_ConvP] = [m for m in self.modules() if isinstance(m, _ConvP)]
        self.flat_params = FlatParams(list(self.parameters()))
        self.flat_params.want_shadow = compute_dtype == torch.bfloat16
        self._shadow_fresh = False
        self._pidx = {id(p): i for i, p in enumerate(self.flat_params.params)}
        self._packs: Dict[int, dict] = {}
        self._pack_table = None
        self._pack_key = None
        self.external_dropout_masks: Optional[List[torch.Tensor]] = None  # parity replay hook
        self.last_dropout_masks: Optional[List[torch.Tensor]] = None
        self.record_dropout_masks = False
        self.dropout_mask_log: List[List[torch.Tensor]] = []   # with record_dropout_masks: one entry per forward (the caller clears it)
        self._drop_calls = 0                  # host mirror of the device call counter below
        self._drop_parity = 0
        self._drop_state: Optional[torch.Tensor] = None   # int64[2] on the device: the call counter (Philox offset = calls << 40), two words used in turn
        # Philox seed of the two dropout sites: drawn from torch's global generator at construction, so a user seed
        # (torch.manual_seed / fix_all_seed) controls it and co-trained models get decorrelated masks (the reference
        # draws every mask from that generator: network.py:165,210).  ddp.FlatGradSync mixes the rank in.
        self.dropout_seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        self._debug: Optional[dict] = None   # tools/debug_unet_layers.py stashes backward intermediates here
        self._grad_hook = None               # data parallelism: called with a bucket index as gradient ranges complete
        self.relu_bits = True                # convolutions keep the ReLU-gate bits of activations whose consumer's data gradient masks by them
        self.pool_codes = True               # max-pool keeps its routing codes for the backward pass (which then does not re-read its input)
        self.wgrad_side_stream = False       # opt-in: weight gradients on a second HIP stream (see _run_backward)
        self.fuse_pool = True                # an encoder block's max pooling rides in its second convolution's call (dct_conv_desc.pool_out)
        self.pool_only = True                # ... whose full-resolution output is then not stored at all (nobody else reads it)
        self.fuse_stem_wgrad = True          # the stem's weight gradient from the epilogue of the data gradient that produces its dy (not stored then)
        self.fuse_skip_grad = True           # the skip connections' bilinear backward gathered by the un-pooling instead of summed in memory
        self.late_packs = True               # the transposed weight packs (first reader: the centre's up-convolution) are launched behind the encoder,
                                             # beside the other chain's kernels, instead of in front of the stem where nothing else runs
        self._pending_packs = None
        self.batch_bias_grads = True         # the four up-convolutions' bias gradients in one launch pair per gradient bucket
        self.batch_skip_resize = True        # the four skip connections' bilinear resizes in one launch, in front of the centre
        self.fuse_drop_pool = True           # the fourth level's dropout + max-pool in one launch (the dropped tensor is never written)
        self._wgrad_stream = None
        self.last_route = {"forward": None, "backward": None}   # the routes of the last passes issued (arch/unet_route.py)

    # ------------------------------------------------------------------------------ weights
    def mark_weights_updated(self, shadow_fresh: bool = False):
        """fp32 masters changed; ``shadow_fresh``: the flat bf16 shadow was rewritten in the same pass (fused Adam)."""
        self._pack_key = None
        self._shadow_fresh = bool(shadow_fresh)

    def repack_in_next_pass(self):
        """The next pass launches the weight packs even if they are current (it is captured, and its replays follow weight updates).
        Current packs were built from a current bf16 shadow, which that pass therefore need not rewrite."""
        fp = self.flat_params
        if fp.is_flat() and self._pack_key == (fp.version, self.compute_dtype, tuple(p._version for p in fp.params)):
            self.mark_weights_updated(shadow_fresh=True)

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self.mark_weights_updated()         # (also drops "the bf16 shadow is fresh": it mirrors the weights before the call)
        return r

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self.mark_weights_updated()
        return r

    def _w(self, conv: _ConvP) -> torch.Tensor:
        return self.flat_params.dense(self._pidx[id(conv.weight)])

    def _gw(self, conv: _ConvP) -> torch.Tensor:
        return self.flat_params.grad_dense(self._pidx[id(conv.weight)])

    def _gb(self, conv: _ConvP) -> torch.Tensor:
        return self.flat_params.grad_dense(self._pidx[id(conv.bias)])

    def _ensure_packs(self, late: bool = False):
        """(Re)build compute-dtype weight packs when the fp32 masters changed.  ``late``: the batched transposing launch is left
        pending for `_run_forward`, which issues it in front of the packs' first reader (`_flush_packs`)."""
        fp = self.flat_params
        if fp.ensure():
            self._shadow_fresh = False
        key = (fp.version, self.compute_dtype, tuple(p._version for p in fp.params))
        if key == self._pack_key:
            return
        dt, dev = self.compute_dtype, fp.flat.device
        use_shadow = dt == torch.bfloat16
        if use_shadow:
            shadow = fp.ensure_shadow()
            if not self._shadow_fresh:          # weights changed outside the fused Adam (init, load, broadcast)
                K.pack_weight(fp.flat, shadow, 1, 1, fp.total)
            self._shadow_fresh = False
        jobs = []
        for conv in self._convs:
            if conv is self.final or conv is self._roles["dec1"][0]:
                continue  # stem and head read the fp32 masters directly
            w = self._w(conv)
            ent = self._packs.get(id(conv))
            if ent is None or ent["dev"] != dev or ent["dt"] != dt:
                ent = {"dev": dev, "dt": dt}
                self._packs[id(conv)] = ent
                self._pack_table = None
                n = w.numel()
                if conv.transposed:
                    ent["fwd"] = torch.empty(n, dtype=dt, device=dev)                    # [(a,b,co)][ci]
                else:
                    ent["dgrad"] = torch.empty(n, dtype=dt, device=dev)                  # [ci][flip taps][co]
            ws = fp.shadow_dense(self._pidx[id(conv.weight)]) if use_shadow else w       # K-major image in dt
            # the packs read the bf16 shadow when there is one (half the bytes of the fp32 masters, same values:
            # both are round-to-nearest of the same fp32 weights)
            if conv.transposed:
                jobs.append((ws, ent["fwd"], conv.cin, 4, conv.cout, 2, False))
                ent["dgrad"] = ws                                                        # [ci][a][b][co] as stored
            else:
                ent["fwd"] = ws                                                          # [co][r][s][ci] as stored
                jobs.append((ws, ent["dgrad"], conv.cout, conv.k * conv.k, conv.cin, 1, True))
        # every transposed pack of the network in one launch (dct_pack_weights_batched); the job table holds device
        # addresses, so it is rebuilt whenever the flat buffer or a pack was re-allocated
        tkey = (fp.version, fp.flat.data_ptr(), fp.shadow.data_ptr() if use_shadow else 0, dev, dt)
        if self._pack_table is None or self._pack_table[0] != tkey:
            self._pack_table = (tkey,) + K.pack_jobs_table(jobs, dev)
        _, table, njobs, tiles, edge = self._pack_table
        self._pending_packs = (table, njobs, tiles, dt, edge)
        if not late:
            self._flush_packs()
        self._pack_key = key

    def _flush_packs(self):
        job, self._pending_packs = self._pending_packs, None
        if job is not None:
            K.pack_weights_batched(*job)

    # ------------------------------------------------------------------------------ forward
    def _check_input(self, x: torch.Tensor):
        if not x.is_cuda:
            raise RuntimeError("dct_amd UNet runs on the HIP device only (no CPU fallback)")
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError(f"expected [B,1,H,W], got {tuple(x.shape)}")
        if min(x.shape[2], x.shape[3]) < 176:
            # same failure the reference has (valid convs): SURVEY.md fact 3
            raise RuntimeError("Kernel size can't be greater than actual input size (UNet needs H,W >= 176)")

    # Autograd-free entry points of the execution plan (the fused trainer step drives them directly: no autograd
    # engine thread hop, and the whole step is a plain launch sequence that a HIP graph can capture).
    def plan_forward(self, x: torch.Tensor, save: bool = True, keep_predrop: bool = False, reuse=None):
        """-> (logits, tape): logits physical NHWC fp32 [B,H,W,C]; tape feeds plan_backward (None if not save).
        ``keep_predrop``: a training pass also keeps the fourth encoder level's output in front of its dropout in the tape.  ``reuse``: the tape
        of such a pass over THE SAME INPUT TENSOR with the same weights: everything in front of the first dropout -- the stem and the eight
        encoder convolutions, half of a forward pass -- is the same computation and is taken from that tape (shared, read-only) instead of
        run again; the pass starts at the fourth level's dropout with masks of its own.  (The FGSM generator's clean forward pass follows the
        joint forward pass of the same network over the same batch: AEGenerator.py:27 behind cotraining_totalloss.py:208-227.)"""
        self._check_input(x)
        facts = self._forward_facts(save, keep_predrop)
        self._ensure_packs(late=facts.late_packs)
        return self._run_forward(x, facts, reuse=reuse)

    supports_grad_overwrite = True
    supports_forward_reuse = True        # plan_forward(keep_predrop=..., reuse=...)

    def plan_backward(self, tape, dlogits: torch.Tensor, need_dx: bool = False, need_dw: bool = True,
                      overwrite: bool = False):
        """dlogits: NHWC fp32 like the logits.  Parameter gradients accumulate into (``overwrite``: replace the
        contents of) the flat gradient buffer (attached as p.grad); returns d/dx as [B,1,H,W] when need_dx."""
        if need_dw:
            self.flat_params.ensure_grads()
        dx = self._run_backward(tape, dlogits, need_dx, need_dw, overwrite=overwrite)
        return dx.reshape(dx.shape[0], 1, dx.shape[1], dx.shape[2]) if dx is not None else None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._check_input(x)
        self._ensure_packs()
        params = self.flat_params.params
        save = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        return _UNetFn.apply(self, save, x, *params)

    def grad_bucket_ranges(self):
        """[lo, hi) element ranges of the flat gradient buffer in the order the backward pass completes them:
        decoder side ("enc*" + final), centre, encoder side ("dec*").  The flat buffer is in registration order
        dec1..dec4, center, enc4..enc1, final, so each bucket is contiguous; the gradient exchange of a bucket can
        start while the rest of the backward still runs (_grad_hook, ddp.FlatGradSync.begin_bucket)."""
        fp = self.flat_params
        first_center = self._pidx[id(self._roles["center"][0].weight)]
        first_enc4 = self._pidx[id(self._roles["enc4"][0].weight)]
        return [(fp.offsets[first_enc4], fp.total), (fp.offsets[first_center], fp.offsets[first_enc4]),
                (0, fp.offsets[first_center])]

    def _side_stream(self, dev):
        if self._wgrad_stream is None or self._wgrad_stream.device != dev:
            self._wgrad_stream = torch.cuda.Stream(device=dev)
        return self._wgrad_stream

    # The plan itself ------------------------------------------------------------------------
    # The two readers of the layout switches and of the network's state (arch/unet_route.py): nothing else in this file asks for them.
    def _forward_facts(self, save: bool, keep_predrop: bool = False) -> ForwardFacts:
        return ForwardFacts(relu_bits=bool(self.relu_bits), pool_codes=bool(self.pool_codes), fuse_pool=bool(self.fuse_pool),
                            pool_only=bool(self.pool_only), fuse_drop_pool=bool(self.fuse_drop_pool),
                            batch_skip_resize=bool(self.batch_skip_resize), late_packs=bool(self.late_packs),
                            save=bool(save), keep_predrop=bool(keep_predrop),
                            net_training=bool(self.training), dropout_on=self.dropout_p > 0, batchnorm=self.batchnorm,
                            masks_external=self.external_dropout_masks is not None, masks_recorded=bool(self.record_dropout_masks),
                            debug=self._debug is not None)

    def _backward_facts(self, forward: ForwardRoute, need_dx: bool, need_dw: bool, overwrite: bool) -> BackwardFacts:
        return BackwardFacts(forward=forward, fuse_skip_grad=bool(self.fuse_skip_grad), fuse_stem_wgrad=bool(self.fuse_stem_wgrad),
                             batch_bias_grads=bool(self.batch_bias_grads), wgrad_side_stream=bool(self.wgrad_side_stream),
                             need_dx=bool(need_dx), need_dw=bool(need_dw), overwrite=bool(overwrite),
                             bf16=self.compute_dtype == torch.bfloat16, batchnorm=self.batchnorm, debug=self._debug is not None,
                             grad_hook_set=self._grad_hook is not None)

    def _run_forward(self, x: torch.Tensor, facts: ForwardFacts, reuse=None):
        """``facts``: `_forward_facts` of this pass (its caller has gathered them: plan_forward needs them for the packs)."""
        dt, dev = self.compute_dtype, x.device
        B, _, H, W = x.shape
        P = self._packs
        A: Dict[str, torch.Tensor] = {}
        xs = x.detach().to(torch.float32).reshape(B, H, W, 1)
        if not xs.is_contiguous():
            xs = xs.contiguous()
        A["x"] = xs
        # a tape to take the encoder from: of the same input tensor, under the same weights (the packs' key), with the pre-dropout tensor and
        # the codes kept; whether this pass may use it is the planner's part
        if (reuse is not None and reuse.get("d4pre") is not None and reuse.get("pack_key") == self._pack_key
                and reuse["x"].data_ptr() == xs.data_ptr() and reuse["x"].shape == xs.shape and all(reuse.get(f"pc{k}") is not None for k in (1, 2, 3))):
            facts = dataclasses.replace(facts, reuse_offered=True)
        route = A["route"] = self.last_route["forward"] = plan_forward_pass(facts)
        p_drop = self.dropout_p

        def new(h, w, c, dtype=dt):
            return torch.empty(B, h, w, c, dtype=dtype, device=dev)

        bn_recs: Dict[str, tuple] = {}

        def bn_relu(raw, bn, name):
            """nn.BatchNorm2d + ReLU of unet_bn: statistics of the raw conv output -> y = relu(scale * raw + shift)."""
            vec = torch.empty(4, bn.num_features, dtype=torch.float32, device=dev)
            y = torch.empty_like(raw)
            K.bn_fwd(raw, bn.weight, bn.bias, bn.eps, bn.momentum, bn.running_mean, bn.running_var,
                     facts.net_training, vec[0], vec[1], vec[2], vec[3], y=y, relu=True)
            bn_recs[name] = (raw, vec, bn)
            return y

        bits: Dict[int, torch.Tensor] = {}     # ReLU-gate bits of the activations whose consumer's data gradient masks by them

        def want_bits(t, bn):
            if not (route.keep_bits and bn is None):
                return None
            b = K.relu_bits_like(t)
            if b is not None:
                bits[id(t)] = b
            return b

        def taped(name):
            """An activation of the tape this pass shares its encoder with, and its gate bits."""
            t = reuse[name]
            if id(t) in reuse["bits"]:
                bits[id(t)] = reuse["bits"][id(t)]
            return t

        def conv3(src, conv, dst, bn=None, name=None, gate=False, pool=(None, None, False)):
            """``gate``: dst feeds a convolution whose data gradient is masked by (dst > 0) -- keep the one-bit image of it.
            ``pool`` = (pooled, codes, only): dst's max pooling (and its routing codes) from the same call; ``only``: dst itself is not stored."""
            K.conv2d(src, P[id(conv)]["fwd"], conv.bias, dst, relu=bn is None, relu_bits_out=want_bits(dst, bn) if gate else None,
                     pool_out=pool[0], pool_codes=pool[1], pool_only=pool[2])
            return dst if bn is None else bn_relu(dst, bn, name)

        masks_out = [] if facts.masks_recorded else None

        def dropout(src, which):
            if route.drop == "none":
                return src
            dst = torch.empty_like(src)
            if route.drop == "external":
                K.dropout_apply(src, dst, self.external_dropout_masks[which], p_drop)
                return dst
            m = torch.empty(src.shape, dtype=torch.uint8, device=dev) if masks_out is not None else None
            state, parity = drop_turn()
            K.dropout_fwd(src, dst, p_drop, self.dropout_seed, 0, mask_out=m, calls_dev=state, parity=parity)
            if masks_out is not None:
                masks_out.append(m)
            return dst

        def drop_turn():
            """-> (device call counter, the word this launch reads); the launch advances the device copy in stream order (graph-replayable)."""
            if self._drop_state is None or self._drop_state.device != dev:
                self._drop_state = torch.tensor([self._drop_calls, self._drop_calls], dtype=torch.int64, device=dev)
                self._drop_parity = 0
            self._drop_calls += 1
            parity = self._drop_parity
            self._drop_parity ^= 1      # (two sites per forward pass: a captured step holds an even number of launches, so its replays stay in turn)
            return self._drop_state, parity

        # encoder ("dec" in the reference's naming)
        h, w = H, W
        src = xs
        for lvl, width in enumerate(_WIDTHS, start=1):
            kind = route.pool[lvl - 1]
            ca, bna, cb, _ = self._roles[f"dec{lvl}"]
            hp, wp = (h - 4 + 1) // 2, (w - 4 + 1) // 2
            if route.reuse:                      # everything in front of the first dropout comes from the tape
                a = taped(f"a{lvl}")
            elif lvl == 1:
                a = new(h - 2, w - 2, width)
                K.conv_cin1_fwd(xs, self._w(ca), ca.bias, a, relu=bna is None, relu_bits_out=want_bits(a, bna))
                if bna is not None:
                    a = bn_relu(a, bna, "a1")
            else:
                a = conv3(src, ca, new(h - 2, w - 2, width), bna, f"a{lvl}", gate=True)
            if kind == "reused":
                d, p, codes = (reuse[f"{k}{lvl}"] for k in ("d", "p", "pc"))
            else:
                # (the dropout + pool launch writes codes whether or not the backward pass will ask for them)
                codes = new(hp, wp, width, torch.uint8) if (route.keep_codes or kind == "dropout_pool") else None
                p = new(hp, wp, width)
                if kind in ("conv", "conv_only"):
                    d = conv3(a, cb, new(h - 4, w - 4, width), pool=(p, codes, kind == "conv_only"))
                    if kind == "conv_only":
                        # nobody reads the block's full-resolution output again (the backward pass routes by the codes and needs its SHAPE):
                        # the buffer goes back to the allocator now instead of riding in the tape until the backward pass (130 MB at level 1)
                        d = _ShapeOf(d)
                elif kind == "dropout_pool":
                    # the fourth level of a training pass: dropout and the pool behind it in one launch; the dropped tensor is never written
                    d = reuse["d4pre"] if route.reuse else conv3(a, cb, new(h - 4, w - 4, width))
                    state, parity = drop_turn()
                    K.dropout_maxpool_fwd(d, p, codes, p_drop, self.dropout_seed, state, parity)
                    if route.keep_d4pre:
                        A["d4pre"], A["pack_key"] = d, self._pack_key        # for a later pass over the same input (plan_forward(reuse=...))
                    d = _ShapeOf(d)
                else:
                    d = conv3(a, cb, new(h - 4, w - 4, width))
                    if lvl == 4:
                        d = dropout(d, 0)
                    K.maxpool_fwd(d, p, codes=codes)
            A[f"a{lvl}"], A[f"d{lvl}"], A[f"p{lvl}"], A[f"pc{lvl}"] = a, d, p, codes
            h, w, src = hp, wp, p
        # center
        self._flush_packs()                  # first reader of a transposed pack: the centre's up-convolution below
        # The four skip connections' resizes (pooled tensor -> second half of the decoder level's concatenation) in ONE launch here, where all
        # four pooled tensors exist, instead of one launch per decoder level (dct_bilinear_fwd_batched)
        cats = {}
        if route.batch_skip_resize:
            ch, cw = h, w
            for lvl, co in ((4, 512), (3, 256), (2, 128), (1, 64)):
                ch, cw = 2 * (ch - 4), 2 * (cw - 4)
                cats[lvl] = new(ch, cw, 2 * co)
            K.bilinear_fwd_batched([A[f"p{lvl}"] for lvl in (4, 3, 2, 1)], [cats[lvl][..., cats[lvl].shape[3] // 2:] for lvl in (4, 3, 2, 1)])

        def up_cat(src, ct, lvl, co):
            """-> decoder level ``lvl``'s concatenation: the up-convolution of src (+ ReLU) in its first ``co`` channels, the resized skip
            connection in the others."""
            cat = cats[lvl] if cats else new(2 * src.shape[1], 2 * src.shape[2], 2 * co)
            K.conv2d(src, P[id(ct)]["fwd"], ct.bias, cat[..., :co], R=1, S=1, relu=True, scatter2x2=True)
            if not cats:
                K.bilinear_fwd(A[f"p{lvl}"], cat[..., co:])
            return cat

        ca, bna, cb, bnb, ct = self._roles["center"]
        c1 = conv3(src, ca, new(h - 2, w - 2, 1024), bna, "c1", gate=True)
        c2 = conv3(c1, cb, new(h - 4, w - 4, 1024), bnb, "c2")
        c2d = dropout(c2, 1)
        cat = up_cat(c2d, ct, 4, 512)
        A["c1"], A["c2"], A["cat4"] = c1, c2d, cat
        # decoder ("enc")
        for lvl, feat, co in ((4, 512, 256), (3, 256, 128), (2, 128, 64)):
            ca, bna, cb, bnb, ct = self._roles[f"enc{lvl}"]
            h, w = cat.shape[1], cat.shape[2]
            ea = conv3(cat, ca, new(h - 2, w - 2, feat), bna, f"e{lvl}a", gate=True)
            eb = conv3(ea, cb, new(h - 4, w - 4, feat), bnb, f"e{lvl}b", gate=True)
            cat = up_cat(eb, ct, lvl - 1, co)
            A[f"e{lvl}a"], A[f"e{lvl}b"], A[f"cat{lvl - 1}"] = ea, eb, cat
        ca, bna, cb, _ = self._roles["enc1"]
        h, w = cat.shape[1], cat.shape[2]
        e1a = conv3(cat, ca, new(h - 2, w - 2, 64), bna, "e1a", gate=True)
        e1b = conv3(e1a, cb, new(h - 4, w - 4, 64))
        f = K.head_fwd(e1b, self._w(self.final), self.final.bias, new(h - 4, w - 4, self.num_classes, torch.float32))
        logits = K.bilinear_fwd(f, new(H, W, self.num_classes, torch.float32))
        A["bn"], A["bn_training"], A["bits"] = bn_recs, facts.net_training, bits
        if bn_recs and facts.net_training:      # nn.BatchNorm2d bookkeeping: one multi-tensor launch for all thirteen layers
            torch._foreach_add_([rec[2].num_batches_tracked for rec in bn_recs.values()], 1)
        A["e1a"], A["e1b"] = e1a, e1b
        A["fshape"] = (h - 4, w - 4)
        if masks_out is not None:
            self.last_dropout_masks = masks_out
            self.dropout_mask_log.append(masks_out)
        A["drop_scale"] = 1.0 / (1.0 - p_drop) if route.scale_by_keep else 1.0
        return logits, (A if facts.save else None)

    def _run_backward(self, A, dlogits: torch.Tensor, need_dx: bool, need_dw: bool, overwrite: bool = False):
        """dlogits: fp32 NHWC [B,H,W,C].  Accumulates parameter grads in place (``overwrite``: writes them -- every
        parameter of the network receives a gradient in every backward pass, so the first pass of a step can replace
        the zero fill of the 124 MB gradient buffer and the read-modify-write of the folds); returns dx or None."""
        route = self.last_route["backward"] = plan_backward_pass(
            self._backward_facts(A["route"], need_dx, need_dw, overwrite))
        gacc = route.accumulate
        dt, dev = self.compute_dtype, dlogits.device
        B = dlogits.shape[0]
        P = self._packs
        C = self.num_classes
        ds = A["drop_scale"]

        def new_like(t, c=None):
            return torch.empty(t.shape[:3] + ((c,) if c else t.shape[3:]), dtype=dt, device=dev)

        # Weight gradients are off the critical path (only the data-gradient chain feeds the next layer): they
        # are queued on a second stream, ordered after the producer of dy by an event, and joined at the end.
        # Their operands stay referenced until the join (`keep`), so the caching allocator cannot hand a dy
        # buffer to a later data-gradient while a weight-gradient kernel still reads it.
        gate_bits = A.get("bits") or {}
        cur = torch.cuda.current_stream(dev)
        side = self._side_stream(dev) if route.side_stream else None
        keep: List[torch.Tensor] = []

        def on_side(*operands):
            if side is None:
                return contextlib.nullcontext()
            side.wait_stream(cur)
            keep.extend(operands)
            return torch.cuda.stream(side)

        stem_fused = [False]

        def conv_bwd(conv, x_in, dy, dx_out, mask=None, mask_channels=0, mask_scale=1.0, accumulate=False, stem=None):
            """dy: grad wrt the conv's pre-activation output (already ReLU-masked).  ``stem``: (x, dw, db, accumulate) -- try to take
            the stem's weight gradient from this data gradient's output tile (dx_out is then not written; stem_fused[0] tells)."""
            if need_dw:
                with on_side(dy, x_in):
                    if route.bias_in_wgrad:      # bias gradient rides along in the weight-gradient launch
                        K.conv2d_wgrad(dy, x_in, self._gw(conv), accumulate=gacc, db=self._gb(conv))
                    else:
                        K.conv2d_wgrad(dy, x_in, self._gw(conv), accumulate=gacc)
                        K.bias_grad(dy, self._gb(conv), accumulate=gacc)
            if dx_out is not None:
                mb = gate_bits.get(id(mask)) if mask is not None else None
                if stem is not None and mb is not None:
                    try:
                        K.conv2d(dy, P[id(conv)]["dgrad"], None, dx_out, pad_h=2, pad_w=2, mask=mask, mask_bits=mb, stem=stem)
                        stem_fused[0] = True
                        return dx_out
                    except K.StemFusionUnsupported:
                        pass                     # (the stem's weight gradient then runs as its own launch)
                K.conv2d(dy, P[id(conv)]["dgrad"], None, dx_out, pad_h=2, pad_w=2, mask=mask,
                         mask_channels=mask_channels, mask_scale=mask_scale, accumulate=accumulate, mask_bits=mb)
            return dx_out

        # The up-convolutions' bias gradients (column sums of their dy, which is the OTHER operand of their weight-gradient GEMM: they cannot ride
        # along there) are collected and summed by ONE launch pair per gradient bucket (dct_bias_grad_batched) instead of one pair per level:
        # six launches of ~5 us less on every model's backward chain.
        pending_bias: List[tuple] = []

        def flush_bias():
            if pending_bias:
                dys, dbs = [t[0] for t in pending_bias], [t[1] for t in pending_bias]
                pending_bias.clear()
                with on_side(*dys):
                    K.bias_grad_batched(dys, dbs, accumulate=gacc)

        def convT_bwd(conv, x_in, dy, dx_out, mask, mask_scale=1.0):
            if need_dw:
                with on_side(dy, x_in):
                    K.conv2d_wgrad(x_in, dy, self._gw(conv), R=2, S=2, stride=2, accumulate=gacc)
                pending_bias.append((dy, self._gb(conv)))
                if not route.batch_bias_grads:
                    flush_bias()
            K.conv2d(dy, P[id(conv)]["dgrad"], None, dx_out, R=2, S=2, stride=2, mask=mask, mask_scale=mask_scale,
                     mask_bits=gate_bits.get(id(mask)))
            return dx_out

        def bn_back(name, g):
            """g: gradient wrt the ReLU output of a BatchNorm'd conv -> gradient wrt the raw conv output (in place)."""
            rec = A["bn"].get(name)
            if rec is None:
                return g
            raw, vec, bn = rec
            c1c2 = torch.empty(2 * bn.num_features, dtype=torch.float32, device=dev)
            K.bn_bwd(raw, g, vec[0], vec[1], vec[2], vec[3],
                     self.flat_params.grad_dense(self._pidx[id(bn.weight)]) if need_dw else None,
                     self.flat_params.grad_dense(self._pidx[id(bn.bias)]) if need_dw else None,
                     c1c2, g, training=A["bn_training"], relu=True, accumulate=gacc)
            return g

        dp: Dict[int, torch.Tensor] = {}            # per encoder level: the gradient at its pooled output
        skip_g: Dict[int, torch.Tensor] = {}

        def skip_bwd(lvl, g):
            """g: the gradient at the resized copy of level ``lvl``'s pooled output (the second half of a concatenation): left for that level's
            un-pooling to gather (K.maxpool_bwd(..., skip=)), or brought back to the pooled size now, where the data gradient will add to it."""
            if route.skip_fused:
                skip_g[lvl] = g
            else:
                dp[lvl] = K.bilinear_bwd(g, new_like(A[f"p{lvl}"]))

        def pooled_bwd(lvl, conv, dy):
            """The data gradient of the convolution that reads level ``lvl``'s pooled output, into dp[lvl] (onto the skip connection's share
            where that was summed in memory)."""
            if route.skip_fused:
                dp[lvl] = new_like(A[f"p{lvl}"])
            conv_bwd(conv, A[f"p{lvl}"], dy, dp[lvl], accumulate=not route.skip_fused)

        fh, fw = A["fshape"]
        df = K.bilinear_bwd(dlogits, torch.empty(B, fh, fw, C, dtype=torch.float32, device=dev))
        e1b, e1a = A["e1b"], A["e1a"]
        de1b = new_like(e1b)
        # (the classifier's weight gradient is a leaf, but launched later -- behind enc1's gradients, out of the stretch where nothing else runs --
        # the step is 0.3 % SLOWER: profiles/r05_dead_zone_ab.txt)
        K.head_bwd(e1b, df, self._w(self.final), de1b,
                   self._gw(self.final) if need_dw else None, self._gb(self.final) if need_dw else None,
                   relu_mask=True, accumulate=gacc)
        ca, _, cb, _ = self._roles["enc1"]
        de1a = bn_back("e1a", conv_bwd(cb, e1a, de1b, new_like(e1a), mask=e1a))
        cat = A["cat1"]
        dcat = conv_bwd(ca, cat, de1a, new_like(cat), mask=cat, mask_channels=64)
        for lvl, co in ((2, 64), (3, 128), (4, 256)):
            ca, _, cb, _, ct = self._roles[f"enc{lvl}"]
            ea, eb = A[f"e{lvl}a"], A[f"e{lvl}b"]
            skip_bwd(lvl - 1, dcat[..., co:])
            deb = bn_back(f"e{lvl}b", convT_bwd(ct, eb, dcat[..., :co], new_like(eb), mask=eb))
            dea = bn_back(f"e{lvl}a", conv_bwd(cb, ea, deb, new_like(ea), mask=ea))
            if self._debug is not None:
                self._debug[f"de{lvl}b"], self._debug[f"de{lvl}a"], self._debug[f"dcat{lvl - 1}"] = deb, dea, dcat
            cat = A[f"cat{lvl}"]
            dcat = conv_bwd(ca, cat, dea, new_like(cat), mask=cat, mask_channels=2 * co)
        if route.bucket_hooks:
            flush_bias()
            self._grad_hook(0)                # decoder-side gradients are complete
        # center (cat4: 512 convT channels + 512 skip channels)
        ca, _, cb, _, ct = self._roles["center"]
        skip_bwd(4, dcat[..., 512:])
        c2d, c1 = A["c2"], A["c1"]
        dc2 = bn_back("c2", convT_bwd(ct, c2d, dcat[..., :512], new_like(c2d), mask=c2d, mask_scale=ds))
        dc1 = bn_back("c1", conv_bwd(cb, c1, dc2, new_like(c1), mask=c1))
        pooled_bwd(4, ca, dc1)
        flush_bias()                          # (the centre's up-convolution was the last one)
        if route.bucket_hooks:
            self._grad_hook(1)                # centre gradients are complete
        # encoder
        dx = None
        for lvl in (4, 3, 2, 1):
            ca, _, cb, _ = self._roles[f"dec{lvl}"]
            a, d = A[f"a{lvl}"], A[f"d{lvl}"]
            dd = K.maxpool_bwd(d, dp[lvl], new_like(d), relu_mask=True, scale=ds if lvl == 4 else 1.0, codes=A[f"pc{lvl}"],
                               skip=skip_g.get(lvl))
            stem = None
            if lvl == 1 and route.try_stem_fusion:
                stem = (A["x"], self._gw(ca), self._gb(ca), gacc)       # the stem's dy has no other reader: see dct_conv_desc.stem_x
            da = bn_back(f"a{lvl}", conv_bwd(cb, a, dd, new_like(a), mask=a, stem=stem))
            if lvl > 1:
                pooled_bwd(lvl - 1, ca, da)
            else:
                if need_dw and not stem_fused[0]:
                    with on_side(da):
                        K.conv_cin1_wgrad(A["x"], da, self._gw(ca), self._gb(ca), accumulate=gacc)
                if need_dx:
                    dx = K.conv_cin1_dgrad(da, self._w(ca), torch.empty_like(A["x"]), pad_h=0, pad_w=0)
        if side is not None:
            cur.wait_stream(side)
        if route.bucket_hooks:
            self._grad_hook(2)                # encoder-side gradients: the whole buffer is final
        return dx


class UNet_bn(UNet):
    """Drop-in for the reference ``UNet_bn`` (network.py:243-290; registry name ``unet_bn``): BatchNorm2d + ReLU after the
    first convolution of every encoder block and of ``enc1``, and after both convolutions of the centre and of the three
    decoder blocks.  Same plan as ``UNet`` with one statistics + one apply pass per BatchNorm (csrc/bn.hip)."""

    def __init__(self, in_channels: int = 1, num_classes: int = 2, compute_dtype=torch.bfloat16, dropout_p: float = 0.5):
        super().__init__(in_channels, num_classes, compute_dtype, dropout_p, batchnorm=True)


class _UNetFn(torch.autograd.Function):
    """One autograd node for the whole network.  Parameter gradients are accumulated directly
    into the net's flat gradient buffer (``p.grad`` views), so ``backward`` returns None for
    them; only d/dx (FGSM, AEGenerator.py:27-28) is returned as a tensor."""

    @staticmethod
    def forward(ctx, net: UNet, save: bool, x: torch.Tensor, *params):
        need_dw = any(p.requires_grad for p in params)
        logits, acts = net._run_forward(x, net._forward_facts(save))
        ctx.net, ctx.acts, ctx.need_dw = net, acts, need_dw
        ctx.set_materialize_grads(False)
        # logical NCHW view of the physical NHWC logits (channels_last strides)
        return logits.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        net: UNet = ctx.net
        n_params = len(net.flat_params.params)
        if g is None or ctx.acts is None:
            return (None, None, None) + (None,) * n_params
        dl = g.permute(0, 2, 3, 1)
        if dl.dtype != torch.float32 or not dl.is_contiguous():
            dl = dl.to(torch.float32).contiguous()
        need_dx = ctx.needs_input_grad[2]
        need_dw = ctx.need_dw and any(ctx.needs_input_grad[3:])
        if need_dw:
            net.flat_params.ensure_grads()
        dx = net._run_backward(ctx.acts, dl, need_dx, need_dw)
        ctx.acts = None
        gx = dx.reshape(dx.shape[0], 1, dx.shape[1], dx.shape[2]) if dx is not None else None
        return (None, None, gx) + (None,) * n_params
