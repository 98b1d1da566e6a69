"""Hand-written HIP ops (gfx950) with autograd: fused BatchNorm(+add+ReLU), 1x1-conv MFMA GEMM with
BatchNorm statistics in its epilogue, LayerNorm, RMSNorm, NHWC max-pool."""
from .batch_norm import FusedBatchNorm2d, batch_norm_act  # noqa: F401
from .layer_norm import FusedLayerNorm, FusedRMSNorm, layer_norm, rms_norm  # noqa: F401
from .pool import FusedMaxPool2d  # noqa: F401
from .conv_bn import conv1x1_bn_act, conv3x3_bn_relu  # noqa: F401
from .dwconv import DepthwiseConv2d, depthwise_conv2d  # noqa: F401
from .window_attention import WindowAttention, window_attention, window_attention_supported  # noqa: F401
# ``ops.cross_entropy`` stays the module (its function is ``ops.cross_entropy.cross_entropy``)
from .cross_entropy import CrossEntropyLoss, MixedTarget  # noqa: F401
from . import onebit  # noqa: F401  (1-bit gradient wire with error feedback: ops.onebit.compress, ...)
from . import powersgd  # noqa: F401  (fused PowerSGD step: ops.powersgd.project, ...)
from . import q8  # noqa: F401  (8-bit block-quantized gradient wire: ops.q8.quantize, ...)
from . import topk  # noqa: F401  (top-k sparsified gradient wire with error feedback: ops.topk.compress, ...)
