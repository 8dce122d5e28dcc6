"""Native (HIP/gfx950) ops and their PyTorch reference fallbacks."""
from . import nn  # noqa: F401
from .loss import cross_entropy, cross_entropy_mix, cross_entropy_with_metrics  # noqa: F401
from .optim import multi_tensor_l2norm  # noqa: F401
