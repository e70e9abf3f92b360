"""Every C of the overlap kernels' dispatch.  tests/test_dice_loss_gpu.py and tests/test_tversky_gpu.py reach C = 2, 3, 4 and 8; the
templates (csrc/loss.hip: overlap_{fin,bwd,bwd_fin}_kernel<C, Rule>) are also instantiated for 5, 6 and 7, where load_px / store_px take
their non-vector paths.  Both families run here at C = 2 ... 8 under both ``per_image`` and both ``accumulate`` values, with the CE term
(and class weights) on and off, the Tversky family with gamma = 1 and gamma = 4/3, through those modules' ``_hold``: the same float64
references and derived bounds, step bit-identical to fwd + bwd, two runs bit-identical.
Shape: B = 3, PPI = 257: two x-blocks per image, the second of one pixel, so fold_rows, wave_fold_rows and block (0, 0)'s finish all run.
The references' preconditions (``TverskyBounds.conditions``, Den - eDen > 0, the sentinel margin) are asserted by ``_hold`` in every case;
the classes were chosen on the CPU so that each case meets them: at C = 2 class 0 is predicted almost perfectly, so gamma != 1 takes
the sentinel class alone there (tests/test_tversky_gpu.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_loss_kernels_scale_gpu import IGN  # noqa: E402
from test_dice_loss_gpu import _classes, _hold as _hold_dice, _inputs, _weights  # noqa: E402
from test_tversky_gpu import P1, P2, _hold as _hold_tversky  # noqa: E402

B, PPI = 3, 257


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


def _case(C):
    g, x, t, sen = _inputs(B, PPI, C, True, seed=PPI + 7 * C + B)
    assert int(((t != IGN) & ((t < 0) | (t >= C))).sum()) >= 3 * B
    return g, x, t, sen


@pytest.mark.parametrize("ce", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("C", [2, 3, 4, 5, 6, 7, 8])
def test_ce_dice_every_c(ops, C, per_image, accumulate, ce):
    g, x, t, sen = _case(C)
    _hold_dice(ops, g, x, t, _weights(C) if ce else None, _classes(C, "fg" if per_image else None), 1e-5, per_image,
               (0.75, 1.0) if ce else (0.0, 1.0), accumulate, sen, "every C")


@pytest.mark.parametrize("abg", [P1, P2])
@pytest.mark.parametrize("ce", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("C", [2, 3, 4, 5, 6, 7, 8])
def test_ce_tversky_every_c(ops, C, per_image, accumulate, ce, abg):
    g, x, t, sen = _case(C)
    which = "s" if C == 2 and abg[2] != 1.0 else ("fg" if per_image else None)
    _hold_tversky(ops, g, x, t, _weights(C) if ce else None, _classes(C, which), 1e-5, abg, per_image, (0.75, 1.0) if ce else (0.0, 1.0),
                  accumulate, sen, "every C")
