"""Loss registry (reference: generalframework/loss/__init__.py:6-16)."""
from .loss import CrossEntropyLoss2d, CrossEntropyDiceLoss2d, DiceLoss, JSD_2D, KL_Divergence_2D, Entropy_2D, softmax_channels  # noqa: F401
from .loss import BoundaryLoss, CrossEntropyBoundaryLoss2d, signed_distance_map  # noqa: F401
from .loss import PseudoLabel_2D, CrossPseudoSupervision_2D, EnsemblePseudoLabel_2D  # noqa: F401
from .loss import SoftPseudoLabel_2D, SoftCrossPseudoSupervision_2D, SoftEnsemblePseudoLabel_2D  # noqa: F401
from .loss import MSEConsistency_2D, CrossMSE_2D, EnsembleMSE_2D  # noqa: F401
from .loss import FocalLoss2d  # noqa: F401
from .loss import TopKCrossEntropyLoss2d  # noqa: F401
from .loss import CrossEntropyTverskyLoss2d, FocalTverskyLoss, TverskyLoss  # noqa: F401
from . import loss as _loss_mod

__all__ = ['get_loss_fn']

LOSS = {'cross_entropy': CrossEntropyLoss2d,
        'focal': FocalLoss2d,
        'topk_ce': TopKCrossEntropyLoss2d,
        'dice': DiceLoss,
        'ce_dice': CrossEntropyDiceLoss2d,
        'tversky': TverskyLoss,
        'focal_tversky': FocalTverskyLoss,
        'ce_tversky': CrossEntropyTverskyLoss2d,
        'boundary': BoundaryLoss,
        'ce_boundary': CrossEntropyBoundaryLoss2d,
        'jsd': JSD_2D,
        'cps': CrossPseudoSupervision_2D,
        'pseudo_label': EnsemblePseudoLabel_2D,
        'soft_cps': SoftCrossPseudoSupervision_2D,
        'soft_pseudo_label': SoftEnsemblePseudoLabel_2D,
        'cross_mse': CrossMSE_2D,
        'mean_mse': EnsembleMSE_2D}


def get_loss_fn(name: str, **kwargs):
    """'mse_2d' and 'partial_ce' of the reference registry are not on the co-training path
     and raise the same ValueError an unknown name raises there."""
    try:
        return LOSS.get(name)(**kwargs)
    except Exception as e:
        raise ValueError('name error when inputting the loss name, with %s' % str(e))


def set_debug_asserts(on: bool):
    _loss_mod.DEBUG_ASSERTS = bool(on)
