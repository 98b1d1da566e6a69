"""DDP communication hooks and their registry (reference: ``ddp_comm_hooks/__init__.py:58-140``)."""
from enum import Enum
from functools import partial

from . import debugging_hooks, default_hooks


def _ddp_comm_hook_wrapper(comm_hook, model, state):
    model.register_comm_hook(state, comm_hook)


def _powerSGD_comm_hook_wrapper(comm_hook, model, state, matrix_approximation_rank, start_powerSGD_iter=1_000):
    from .powerSGD_hook import PowerSGDState

    st = PowerSGDState(process_group=state, matrix_approximation_rank=matrix_approximation_rank,
                       start_powerSGD_iter=start_powerSGD_iter)
    model.register_comm_hook(st, comm_hook)


def _fused_powerSGD_comm_hook_wrapper(comm_hook, model, state, matrix_approximation_rank, start_powerSGD_iter=1_000):
    from .powersgd_fused_hook import FusedPowerSGDState

    st = FusedPowerSGDState(process_group=state, matrix_approximation_rank=matrix_approximation_rank,
                            start_powerSGD_iter=start_powerSGD_iter)
    model.register_comm_hook(st, comm_hook)


def _lazy(modname, attr):
    def f(*a, **k):
        import importlib

        return getattr(importlib.import_module(f"{__name__}.{modname}"), attr)(*a, **k)

    f.__name__ = attr
    f.__qualname__ = attr
    return f


def __getattr__(name):
    # comm_hooks.Q8State / comm_hooks.q8_allreduce_hook, imported on first use like the hooks above;
    # registered with ``model.register_comm_hook(Q8State(...), q8_allreduce_hook)``
    if name in ("Q8State", "q8_allreduce_hook"):
        from . import q8_hook

        return getattr(q8_hook, name)
    if name in ("OneBitState", "onebit_allreduce_hook"):
        from . import onebit_hook

        return getattr(onebit_hook, name)
    if name in ("TopKState", "topk_allreduce_hook"):
        from . import topk_hook

        return getattr(topk_hook, name)
    if name in ("FusedPowerSGDState", "fused_powerSGD_hook"):
        from . import powersgd_fused_hook

        return getattr(powersgd_fused_hook, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


class DDPCommHookType(Enum):
    ALLREDUCE = partial(_ddp_comm_hook_wrapper, comm_hook=default_hooks.allreduce_hook)
    FP16_COMPRESS = partial(_ddp_comm_hook_wrapper, comm_hook=default_hooks.fp16_compress_hook)
    BF16_COMPRESS = partial(_ddp_comm_hook_wrapper, comm_hook=default_hooks.bf16_compress_hook)
    QUANTIZE_PER_TENSOR = partial(_ddp_comm_hook_wrapper,
                                  comm_hook=_lazy("quantization_hooks", "quantization_pertensor_hook"))
    QUANTIZE_PER_CHANNEL = partial(_ddp_comm_hook_wrapper,
                                   comm_hook=_lazy("quantization_hooks", "quantization_perchannel_hook"))
    POWER_SGD = partial(_powerSGD_comm_hook_wrapper, comm_hook=_lazy("powerSGD_hook", "powerSGD_hook"),
                        matrix_approximation_rank=1)
    POWER_SGD_RANK2 = partial(_powerSGD_comm_hook_wrapper, comm_hook=_lazy("powerSGD_hook", "powerSGD_hook"),
                              matrix_approximation_rank=2)
    BATCHED_POWER_SGD = partial(_powerSGD_comm_hook_wrapper,
                                comm_hook=_lazy("powerSGD_hook", "batched_powerSGD_hook"),
                                matrix_approximation_rank=1)
    FUSED_POWER_SGD = partial(_fused_powerSGD_comm_hook_wrapper,
                              comm_hook=_lazy("powersgd_fused_hook", "fused_powerSGD_hook"),
                              matrix_approximation_rank=1)
    NOOP = partial(_ddp_comm_hook_wrapper, comm_hook=debugging_hooks.noop_hook)


def register_ddp_comm_hook(comm_hook_type: DDPCommHookType, model, state=None):
    comm_hook_type.value(model=model, state=state)
