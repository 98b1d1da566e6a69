from .datasets import CIFAR10Binary, SyntheticImages  # noqa: F401
from .mixup import MixPlan, Mixup, mix_images  # noqa: F401
from .packing import PackedDocs, packed_docs, packed_docs_from_ids, packed_labels  # noqa: F401
from .sampler import DistributedSampler  # noqa: F401
