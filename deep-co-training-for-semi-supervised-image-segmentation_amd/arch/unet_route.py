"""The route of one UNet pass: every layout decision, taken once, before anything is launched (tables: DESIGN.md 4.3).

Pure Python over plain values -- no torch, no HIP -- so the decision table is tested on the CPU (tests/test_host_logic_cpu.py).
``UNet._forward_facts`` / ``_backward_facts`` read the network's switches and the facts of the call;
``plan_forward_pass`` / ``plan_backward_pass`` turn them into a frozen route that ``UNet._run_forward`` / ``_run_backward`` follow
without asking again.  The forward route rides in the tape (``tape["route"]``): the backward pass is planned from what the forward
pass DID, not from what the switches say by then.

Forward route (lvl: encoder level 1..4; ``plain`` = no external masks, no recorded masks, no debug stash):

  training       net_training and dropout_on
  drop           "external" if masks_external, else "device" if training, else "none"
  scale_by_keep  drop != "none"                       (the centre's backward scales by 1 / (1 - p))
  keep_bits      save and relu_bits                   (per tensor: only where K.relu_bits_like has a buffer and no BatchNorm follows)
  keep_codes     save and pool_codes
  reuse          reuse_offered and training and not batchnorm and plain
  pool[lvl - 1]  reuse:            "reused" below level 4, "dropout_pool" (fed from the tape's d4pre) at level 4
                 else, with fuse = fuse_pool and not (lvl == 4 and drop != "none"):
                   "conv_only"     fuse and pool_only and (keep_codes or not save) and not debug
                   "conv"          fuse otherwise
                   "dropout_pool"  lvl == 4 and training and fuse_drop_pool and keep_codes and plain
                   "separate"      everything else
  keep_d4pre     pool[3] == "dropout_pool" and keep_predrop and save and not reuse
  batch_skip_resize, late_packs   the switches, copied through

Backward route:

  side_stream      need_dw and wgrad_side_stream
  accumulate       not (overwrite and need_dw)
  bias_in_wgrad    bf16
  skip_fused       fuse_skip_grad and the forward pass kept codes on all four levels (keep_codes, or reuse: its tape had them)
  try_stem_fusion  need_dw and not need_dx and fuse_stem_wgrad and bf16 and not side_stream and not batchnorm and not debug
                   (at the launch two fall-backs remain: no gate bits for a1, and the library's StemFusionUnsupported)
  bucket_hooks     need_dw and grad_hook_set and not side_stream
  batch_bias_grads the switch, copied through
"""
from __future__ import annotations

import dataclasses
from typing import Tuple


@dataclasses.dataclass(frozen=True)
class ForwardFacts:
    # the forward pass's switches: UNet attributes of the same names
    relu_bits: bool = True
    pool_codes: bool = True
    fuse_pool: bool = True
    pool_only: bool = True
    fuse_drop_pool: bool = True
    batch_skip_resize: bool = True
    late_packs: bool = True
    # the call
    save: bool = True
    keep_predrop: bool = False
    reuse_offered: bool = False                 # a tape was handed in and matches: d4pre and pc1..3 present, same packs, same input tensor
    # the network
    net_training: bool = True
    dropout_on: bool = True                     # dropout_p > 0
    batchnorm: bool = False
    masks_external: bool = False                # external_dropout_masks is not None
    masks_recorded: bool = False                # record_dropout_masks
    debug: bool = False                         # _debug is not None


@dataclasses.dataclass(frozen=True)
class ForwardRoute:
    training: bool
    drop: str                                   # none | device | external
    scale_by_keep: bool
    keep_bits: bool
    keep_codes: bool
    reuse: bool
    pool: Tuple[str, str, str, str]             # per encoder level: reused | conv | conv_only | dropout_pool | separate
    keep_d4pre: bool
    batch_skip_resize: bool
    late_packs: bool


@dataclasses.dataclass(frozen=True)
class BackwardFacts:
    forward: ForwardRoute                       # the route the tape was recorded under
    # the backward pass's switches
    fuse_skip_grad: bool = True
    fuse_stem_wgrad: bool = True
    batch_bias_grads: bool = True
    wgrad_side_stream: bool = False
    # the call
    need_dx: bool = False
    need_dw: bool = True
    overwrite: bool = False
    # the network
    bf16: bool = True
    batchnorm: bool = False
    debug: bool = False
    grad_hook_set: bool = False                 # _grad_hook is not None


@dataclasses.dataclass(frozen=True)
class BackwardRoute:
    side_stream: bool
    accumulate: bool
    bias_in_wgrad: bool
    skip_fused: bool
    try_stem_fusion: bool
    bucket_hooks: bool
    batch_bias_grads: bool


def plan_forward_pass(f: ForwardFacts) -> ForwardRoute:
    training = bool(f.net_training and f.dropout_on)
    drop = "external" if f.masks_external else "device" if training else "none"
    keep_codes = bool(f.save and f.pool_codes)
    # the masks are drawn on the device and nobody asks for them or for intermediates: what the dropout + pool launch and a shared encoder need
    plain = not (f.masks_external or f.masks_recorded or f.debug)
    reuse = bool(f.reuse_offered and training and not f.batchnorm and plain)

    def pool(lvl):
        if reuse:
            return "reused" if lvl < 4 else "dropout_pool"
        # the pool reads the convolution's output as it is (no dropout in between: every level but the fourth of a pass that drops)
        if f.fuse_pool and not (lvl == 4 and drop != "none"):
            # ... and alone: the backward pass routes by the codes and never reads the block's full-resolution output
            return "conv_only" if (f.pool_only and (keep_codes or not f.save) and not f.debug) else "conv"
        if lvl == 4 and training and f.fuse_drop_pool and keep_codes and plain:
            return "dropout_pool"
        return "separate"

    pools = tuple(pool(lvl) for lvl in (1, 2, 3, 4))
    return ForwardRoute(training=training, drop=drop, scale_by_keep=drop != "none", keep_bits=bool(f.save and f.relu_bits),
                        keep_codes=keep_codes, reuse=reuse, pool=pools,
                        keep_d4pre=bool(pools[3] == "dropout_pool" and f.keep_predrop and f.save and not reuse),
                        batch_skip_resize=bool(f.batch_skip_resize), late_packs=bool(f.late_packs))


def plan_backward_pass(f: BackwardFacts) -> BackwardRoute:
    side = bool(f.need_dw and f.wgrad_side_stream)
    return BackwardRoute(side_stream=side, accumulate=not (f.overwrite and f.need_dw), bias_in_wgrad=bool(f.bf16),
                         skip_fused=bool(f.fuse_skip_grad and (f.forward.keep_codes or f.forward.reuse)),
                         try_stem_fusion=bool(f.need_dw and not f.need_dx and f.fuse_stem_wgrad and f.bf16 and not side and
                                              not f.batchnorm and not f.debug),
                         bucket_hooks=bool(f.need_dw and f.grad_hook_set and not side),
                         batch_bias_grads=bool(f.batch_bias_grads))
