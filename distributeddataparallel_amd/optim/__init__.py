from .fused import (FusedAdam, FusedAdamW, FusedSGD, clip_grad_norm_, grad_norm,  # noqa: F401
                    stochastic_round_bf16)
from .layerwise import FusedLAMB, FusedLARS  # noqa: F401
