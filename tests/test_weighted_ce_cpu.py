"""``CrossEntropyLoss2d`` takes the reference's ``weight`` / ``reduce`` / ``size_average`` arguments (the kernels behind them:
tests/test_weighted_ce_gpu.py); without a device it still refuses CPU tensors.  Header, exports and binding table of the five
``dct_ce_weighted_*`` / ``dct_ce_map_*`` symbols are covered by tests/test_abi_cpu.py."""
import pytest
import torch


def test_constructs_with_weights_and_reductions():
    from dct_amd.loss import CrossEntropyLoss2d, get_loss_fn
    w = [0.1, 1, 2.5, 0]
    crit = CrossEntropyLoss2d(weight=w)
    assert crit.weight is w and crit.reduction == "mean" and crit.ignore_index == 255
    assert get_loss_fn("cross_entropy", weight=w).weight is w
    wt = torch.tensor(w)
    assert CrossEntropyLoss2d(weight=wt).weight is wt
    assert CrossEntropyLoss2d(reduce=False).reduction == "none"
    assert CrossEntropyLoss2d(reduce=False, size_average=False).reduction == "none"
    assert CrossEntropyLoss2d(size_average=False).reduction == "sum"
    assert CrossEntropyLoss2d(weight=w, size_average=False, ignore_index=7).ignore_index == 7
    # no device copy of the weights exists before the first call; None / all ones need none at all
    assert CrossEntropyLoss2d().device_weight("cuda:0") is None and CrossEntropyLoss2d(weight=[1, 1.0]).device_weight("cuda:0", 2) is None


@pytest.mark.parametrize("kw", [dict(), dict(weight=[0.1, 1, 2.5, 0]), dict(reduce=False), dict(size_average=False)])
def test_cpu_tensors_are_still_rejected(kw):
    from dct_amd.loss import CrossEntropyLoss2d
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CrossEntropyLoss2d(**kw)(torch.zeros(1, 4, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64))


def test_weight_length_is_checked_against_the_logits():
    from dct_amd.loss import CrossEntropyLoss2d
    with pytest.raises(ValueError, match="3 class weights for logits of 4 classes"):
        CrossEntropyLoss2d(weight=[1, 2, 3]).device_weight("cuda:0", 4)
    with pytest.raises(ValueError, match="class weights"):
        CrossEntropyLoss2d(weight=[1, 1, 1]).device_weight("cuda:0", 4)
