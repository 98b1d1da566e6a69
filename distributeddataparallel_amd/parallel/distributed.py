"""``DistributedDataParallel`` — the user-facing DDP wrapper over the native xddp Reducer.

API and behaviour follow the reference stack's wrapper (SURVEY.md §2.2 T6a–T6m,
``torch/nn/parallel/distributed.py:328-2434``, used by ``ref:dpp.py:39``):

* constructor signature (``device_ids``, ``broadcast_buffers``, ``bucket_cap_mb``,
  ``find_unused_parameters``, ``gradient_as_bucket_view``, ``static_graph``, ...);
* init-time parameter verification + rank-0 broadcast of params and buffers;
* iteration 0 uses one bucket (or [1 MiB, cap] with ``find_unused_parameters``), then the
  buckets are rebuilt once in gradient-ready order;
* per-forward buffer broadcast, ``no_sync()``, ``join()``, comm hooks, static graph,
  ``module.``-prefixed ``state_dict`` (the wrapped net lives in ``self.module``).

MI355X additions:

* ``bucket_policy`` — with ``bucket_cap_mb=None`` on the RCCL backend the rebuilt buckets follow
  the xGMI policy of ``parallel/bucket_policy.py`` (small first bucket, large middle buckets for
  big models, a small LAST bucket so the all-reduce exposed after backward is short). An
  explicit ``bucket_cap_mb`` (or ``XDDP_BUCKET_CAP_MB``) keeps the reference semantics exactly;
* ``comm_dtype`` — communicate gradients in bf16/fp16 with a fused cast inside the bucket
  pack kernel (the builtin ``BF16_COMPRESS`` hook without a Python round trip).
"""
from __future__ import annotations

import copy
import logging
import os
import sys
import weakref
from contextlib import contextmanager
from enum import Enum, auto
from typing import Any, Callable, List, Optional

import torch
import torch.nn as nn
from torch.autograd.profiler import record_function

from .. import distributed as xdist
from .._native import load
from ..ops import linear as _linear_ops
from ..utils import fault as _fault
from ..utils import replicas as _replicas
from . import bucket_policy as _bp
from .join import Join, Joinable, JoinHook

logger = logging.getLogger(__name__)

DEFAULT_FIRST_BUCKET_BYTES = 1024 * 1024
DEFAULT_BUCKET_CAP_MB = 25
BROADCAST_BUCKET_BYTES = 250 * 1024 * 1024

__all__ = ["DistributedDataParallel", "BuiltinCommHookType", "BufferCommHookLocation"]


class BuiltinCommHookType(Enum):
    ALLREDUCE = auto()
    FP16_COMPRESS = auto()
    BF16_COMPRESS = auto()


class BufferCommHookLocation(Enum):
    """Where a buffer comm hook runs (reference ``_BufferCommHookLocation``)."""
    PRE_FORWARD = auto()
    POST_FORWARD = auto()


_BufferCommHookLocation = BufferCommHookLocation


def _find_tensors(obj) -> List[torch.Tensor]:
    if isinstance(obj, torch.Tensor):
        return [obj]
    if isinstance(obj, (list, tuple)):
        return [t for o in obj for t in _find_tensors(o)]
    if isinstance(obj, dict):
        return [t for o in obj.values() for t in _find_tensors(o)]
    if hasattr(obj, "__dataclass_fields__"):
        return [t for f in obj.__dataclass_fields__ for t in _find_tensors(getattr(obj, f))]
    return []


def _to_device(obj, device, non_blocking=True):
    if isinstance(obj, torch.Tensor):
        return obj if obj.device == device else obj.to(device, non_blocking=non_blocking)
    if isinstance(obj, tuple) and hasattr(obj, "_fields"):
        return type(obj)(*(_to_device(o, device, non_blocking) for o in obj))
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_device(o, device, non_blocking) for o in obj)
    if isinstance(obj, dict):
        return {k: _to_device(v, device, non_blocking) for k, v in obj.items()}
    return obj


class _CastParams(torch.autograd.Function):
    """All parameters -> ``dtype`` copies in one multi-tensor launch; grads back in one launch."""

    @staticmethod
    def forward(ctx, dtype, *params):
        ctx.src_dtypes = [p.dtype for p in params]
        outs = [torch.empty_like(p, dtype=dtype) for p in params]
        _mt_copy(list(params), outs)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        idx = [i for i, g in enumerate(grads) if g is not None]
        res = [None] * len(grads)
        src = [_dense(grads[i]) for i in idx]
        dst = [torch.empty_like(g, dtype=ctx.src_dtypes[i]) for i, g in zip(idx, src)]
        _mt_copy(src, dst)
        for i, d in zip(idx, dst):
            res[i] = d
        return (None, *res)


def tail_chunks(numel: int, element_size: int, chunk_bytes: int) -> List[tuple]:
    """Element ranges [lo, hi) splitting a flat bucket into collectives of ~``chunk_bytes``; every
    boundary is a multiple of 4096 elements (16-B aligned for any dtype). Identical on every rank:
    it depends on the bucket's size only."""
    step = max(4096, (chunk_bytes // max(1, element_size)) // 4096 * 4096)
    if numel <= 2 * step:
        return [(0, numel)]
    return [(lo, min(numel, lo + step)) for lo in range(0, numel, step)]


def _dense(t: torch.Tensor) -> torch.Tensor:
    if t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)):
        return t
    return t.contiguous()


def _mt_copy(src: List[torch.Tensor], dst: List[torch.Tensor]):
    """dtype-converting copy of a tensor list: one HIP launch per (src, dst) dtype pair on GPU."""
    if not src:
        return
    if src[0].is_cuda:
        groups = {}
        for a, b in zip(src, dst):
            groups.setdefault((a.dtype, b.dtype), ([], []))
            groups[(a.dtype, b.dtype)][0].append(a)
            groups[(a.dtype, b.dtype)][1].append(b)
        for a, b in groups.values():
            load().mt_scale_copy(a, b, 1.0)
    else:
        with torch.no_grad():
            for a, b in zip(src, dst):
                b.copy_(a)


class _DDPJoinHook(JoinHook):
    """Shadows one DDP iteration's collectives on a rank that ran out of inputs."""

    def __init__(self, ddp: "DistributedDataParallel", divide_by_initial_world_size: bool):
        self.ddp = ddp
        self.ddp._divide_by_initial_world_size = divide_by_initial_world_size

    def main_hook(self):
        """Mirror, in order, the collectives one training iteration of a non-joined rank issues
        (reference ``_DDPJoinHook.main_hook``): rebuild broadcast, buffer broadcast, the
        "will you sync backward" flag, then one all-reduce per bucket with the same reduction
        op and the unused-parameter bitmap — or nothing more when that iteration does not sync."""
        ddp = self.ddp
        ddp.reducer.rebuild_buckets()
        # buffers go through the same hook-or-broadcast helper, at the same place, as on the
        # training ranks: PRE_FORWARD (or the default broadcast) before the sync flag, a
        # POST_FORWARD hook after it
        if ddp._check_sync_bufs_pre_fwd():
            ddp._sync_buffers(joined=True)
        should_sync = ddp._check_global_requires_backward_grad_sync(is_joined_rank=True)
        if ddp._check_sync_bufs_post_fwd():
            ddp._sync_buffers(joined=True)
        # a skipped-sync iteration means the next forward does not broadcast buffers either
        ddp.require_forward_param_sync = should_sync
        if not should_sync:
            return
        ddp.reducer.shadow_allreduce_buckets(premul_sum=not ddp._divide_by_initial_world_size)
        if ddp.find_unused_parameters:
            m = torch.zeros(len(ddp._module_parameters), dtype=torch.int32, device=ddp._comm_device)
            ddp.process_group.allreduce(m, xdist.ReduceOp.SUM).wait()
        # a rank that joined before finishing an iteration has no grad-ready order; seed one so
        # it takes part in the rebuild broadcast the other ranks issue at their next forward
        ddp.reducer.push_all_rebuilt_params()

    def post_hook(self, is_last_joiner: bool):
        self.ddp._sync_final_model(is_last_joiner)


def _python_reducer_mode() -> bool:
    """XDDP_PYTHON_REDUCER=1, or torch._dynamo's ``optimize_ddp`` set to "python_reducer" (only
    consulted when dynamo is already imported: importing it costs seconds)."""
    if os.environ.get("XDDP_PYTHON_REDUCER", "0") == "1":
        return True
    dyn = sys.modules.get("torch._dynamo")
    if dyn is None:
        return False
    try:
        return dyn.utils.get_optimize_ddp_mode() == "python_reducer"
    except Exception:  # older/newer dynamo without the helper
        return False


class DistributedDataParallel(nn.Module, Joinable):
    def __init__(
        self,
        module: nn.Module,
        device_ids: Optional[List[Any]] = None,
        output_device=None,
        dim: int = 0,
        broadcast_buffers: bool = True,
        init_sync: bool = True,
        process_group=None,
        bucket_cap_mb: Optional[float] = None,
        find_unused_parameters: bool = False,
        check_reduction: bool = False,
        gradient_as_bucket_view: bool = False,
        static_graph: bool = False,
        delay_all_reduce_named_params=None,
        param_to_hook_all_reduce=None,
        mixed_precision=None,
        device_mesh=None,
        skip_all_reduce_unused_params: bool = False,
        comm_dtype: Optional[torch.dtype] = None,
        first_bucket_cap_mb: Optional[float] = None,
        bucket_policy: Optional[str] = None,
        python_reducer: Optional[bool] = None,
    ):
        super().__init__()
        Joinable.__init__(self)
        C = load()
        if (delay_all_reduce_named_params is None) != (param_to_hook_all_reduce is None):
            raise ValueError("delay_all_reduce_named_params and param_to_hook_all_reduce need to be set at the "
                             "same time.")
        if device_mesh is not None:
            if process_group is not None:
                raise RuntimeError("Cannot specify both process_group and device_mesh arguments.")
            process_group = self._group_from_mesh(device_mesh)
        self.process_group = self._resolve_process_group(process_group)
        self.skip_all_reduce_unused_params = skip_all_reduce_unused_params
        self.module = module
        self.dim = dim
        self.broadcast_buffers = broadcast_buffers
        self.find_unused_parameters = find_unused_parameters
        self.gradient_as_bucket_view = gradient_as_bucket_view
        self.require_backward_grad_sync = True
        self.require_forward_param_sync = True
        self.static_graph = False
        self._divide_by_initial_world_size = True
        # XDDP_CHECK_REPLICAS=N: every N-th forward compares a checksum of every parameter (and of the
        # synced buffers) across ranks and raises naming the diverged ranks (utils/replicas.py)
        self._check_replicas_every = int(os.environ.get("XDDP_CHECK_REPLICAS", "0") or 0)
        self.mixed_precision = mixed_precision
        if mixed_precision is not None:
            self._setup_mixed_precision(module, mixed_precision)
            red = getattr(mixed_precision, "reduce_dtype", None)
            if comm_dtype is None and red is not None and red != torch.float32:
                comm_dtype = red  # reduce in reduce_dtype through the fused pack/cast kernel

        self._params_and_buffers_to_ignore = set(getattr(module, "_ddp_params_and_buffers_to_ignore", []))
        self._delay_all_reduce_params = []
        if delay_all_reduce_named_params is not None:
            for name, param in delay_all_reduce_named_params:
                self._params_and_buffers_to_ignore.add(name)
                self._delay_all_reduce_params.append(param)
        named = [(n, p) for n, p in module.named_parameters() if n not in self._params_and_buffers_to_ignore]
        seen = set()
        self._module_parameters, self._param_names = [], []
        for n, p in named:
            if p.requires_grad and id(p) not in seen:
                seen.add(id(p))
                self._module_parameters.append(p)
                self._param_names.append(n)
        self._delay_all_reduce_all_params = not self._module_parameters and bool(self._delay_all_reduce_params)
        if not self._module_parameters and not self._delay_all_reduce_params:
            raise RuntimeError("DistributedDataParallel is not needed when a module doesn't have any parameter "
                               "that requires a gradient.")
        devices = {p.device for p in (self._module_parameters or self._delay_all_reduce_params)}
        if len(devices) > 1:
            raise ValueError(f"DistributedDataParallel's input module must be on a single device, found {devices}")
        self._param_device = next(iter(devices))
        self.device_type = self._param_device.type
        if device_ids is not None and len(device_ids) > 1:
            raise ValueError("device_ids can only be None or contain a single element.")
        if self.device_type == "cpu" or device_ids is None or len(device_ids) == 0:
            self.device_ids = None
            self.output_device = None
        else:
            self.device_ids = [torch.device("cuda", d) if isinstance(d, int) else torch.device(d) for d in device_ids]
            self.output_device = self.device_ids[0] if output_device is None else torch.device(output_device)
        if self.process_group.backend == "rccl" and self.device_type != "cuda":
            raise ValueError("the rccl backend needs the module on a GPU")
        # backend "cpu" with a GPU module: collectives are staged through host memory (slow;
        # used to run several DDP ranks on one GPU, where RCCL refuses duplicate devices)
        self._comm_device = self._param_device

        total_bytes = sum(p.numel() * p.element_size() for p in self._module_parameters)
        if comm_dtype is not None:
            total_bytes = sum(p.numel() for p in self._module_parameters) * torch.empty(0, dtype=comm_dtype).element_size()
        from ..distributed import calibrate as _cal

        if self.device_type == "cuda" and _cal.enabled(self.process_group):
            # XDDP_COMM_CALIBRATE=1: measure alpha / B and the per-size route (RCCL ring vs the peer
            # kernels) at the sizes this job's buckets will have, before the plan is fixed
            plan0, _ = _bp.resolve_plan(bucket_policy, bucket_cap_mb, first_bucket_cap_mb, total_bytes,
                                        self.process_group.size(), self.process_group.backend)
            sizes = _cal.probe_sizes(plan0.first_bytes, plan0.cap_bytes, plan0.tail_bytes, total_bytes)
            cdt = comm_dtype or (self._module_parameters or self._delay_all_reduce_params)[0].dtype
            _cal.calibrate(self.process_group, sizes, cdt)
        self.comm_calibration = getattr(self.process_group, "comm_calibration", None)
        self.bucket_plan, _ = _bp.resolve_plan(bucket_policy, bucket_cap_mb, first_bucket_cap_mb, total_bytes,
                                               self.process_group.size(), self.process_group.backend)
        self.bucket_bytes_cap = self.bucket_plan.cap_bytes
        self.first_bucket_bytes_cap = self.bucket_plan.first_bytes
        self.broadcast_bucket_size = BROADCAST_BUCKET_BYTES
        self._comm_dtype = comm_dtype

        self._buffers_list = [b for n, b in module.named_buffers() if n not in self._params_and_buffers_to_ignore]
        self._comm_hooks = []
        self._use_python_reducer, self._accum_grad_hooks = False, []
        self._logging_sample_rate = 100
        self._delay_grad_buffer = None
        self._delay_grad_views: List[torch.Tensor] = []
        if self._delay_all_reduce_params:
            self._register_delay_all_reduce_hook(param_to_hook_all_reduce)
        if self._delay_all_reduce_all_params:
            self.reducer = None
            return
        if init_sync:
            C.verify_params_across_processes(self.process_group.comm, self._module_parameters)
            self._sync_module_states(src=0)

        self._build_reducer()
        if static_graph:
            self._set_static_graph()
        self._use_python_reducer = _python_reducer_mode() if python_reducer is None else bool(python_reducer)
        self._accum_grad_hooks = []
        if self._use_python_reducer:
            self._register_accum_grad_hook()

    # ----------------------------------------------------------------------------- python reducer
    def _register_accum_grad_hook(self):
        """T6k, the compiled-autograd "python reducer" (``pt:nn/parallel/distributed.py:954-986``):
        no bucketing Reducer; each parameter's post-accumulate-grad hook reduces its own gradient
        (AVG) or hands ``(grad, param)`` to the registered comm hooks. The all-reduces are launched
        asynchronously on the communicator's stream as the gradients arrive, and one end-of-backward
        callback makes the compute stream wait for all of them (torch's version blocks per
        parameter through a functional all-reduce + copy)."""
        ref = weakref.ref(self)
        pending = []

        def finish():
            works = list(pending)
            pending.clear()
            for w in works:
                w.wait()

        def hook(param):
            ddp = ref()
            if ddp is None or not ddp.require_backward_grad_sync or param.grad is None:
                return
            if ddp._comm_hooks:
                for state, h in ddp._comm_hooks:
                    h(state, (param.grad, param))
                return
            if not pending:
                torch.autograd.Variable._execution_engine.queue_callback(finish)
            pending.append(ddp.process_group.allreduce(param.grad, xdist.ReduceOp.AVG))

        for p in self._module_parameters:
            self._accum_grad_hooks.append(p.register_post_accumulate_grad_hook(hook))

    # ----------------------------------------------------------------------------- delayed all-reduce
    def _register_delay_all_reduce_hook(self, param_to_hook_all_reduce):
        """T6j (``pt:nn/parallel/distributed.py:988-1036``): the listed params leave the Reducer;
        their grads live in one flat buffer that is all-reduced (AVG) when the hook parameter's
        gradient has been accumulated; backward's end waits for it on the compute stream."""
        params = self._delay_all_reduce_params
        dts = {p.dtype for p in params}
        if len(dts) != 1:
            raise ValueError(f"delayed all-reduce params must share one dtype, got {dts}")
        self._delay_grad_buffer = torch.zeros(sum(p.numel() for p in params), dtype=dts.pop(), device=params[0].device)
        load().broadcast_coalesced(self.process_group.comm, [p.detach() for p in params], self.broadcast_bucket_size, 0)
        off = 0
        for p in params:
            self._delay_grad_views.append(self._delay_grad_buffer[off:off + p.numel()].view(p.shape))
            off += p.numel()
        ref = weakref.ref(self)
        self._delay_state = {"arrived": 0, "work": None, "queued": False}
        n_grad = sum(1 for p in params if p.requires_grad)

        def launch(ddp):
            st = ddp._delay_state
            if st["work"] is None:
                st["work"] = ddp.process_group.allreduce(ddp._delay_grad_buffer, xdist.ReduceOp.AVG)

        def finish():
            ddp = ref()
            if ddp is None:
                return
            launch(ddp)  # a delayed param unused this iteration: reduce what arrived
            ddp._delay_state["work"].wait()
            ddp._delay_state.update(arrived=0, work=None, queued=False)

        def hook(_param):
            ddp = ref()
            if ddp is None or not ddp.require_backward_grad_sync:
                return
            st = ddp._delay_state
            st["arrived"] += 1
            if not st["queued"]:
                st["queued"] = True
                torch.autograd.Variable._execution_engine.queue_callback(finish)
            if st["arrived"] == n_grad:  # every delayed grad is in the buffer: overlap the rest of backward
                launch(ddp)

        # ``param_to_hook_all_reduce`` is the reference's trigger; launching once every delayed
        # grad has been accumulated (its hook included) avoids reducing a half-filled buffer
        self._delay_hook_handles = [p.register_post_accumulate_grad_hook(hook) for p in params if p.requires_grad]
        if not param_to_hook_all_reduce.requires_grad:
            raise ValueError("param_to_hook_all_reduce must require grad")

    def _clear_grad_buffer(self):
        """Point the delayed params' .grad at their buffer views before backward."""
        if self._delay_grad_buffer is None:
            return
        all_none = all(p.grad is None for p in self._delay_all_reduce_params)
        for i, p in enumerate(self._delay_all_reduce_params):
            if p.grad is None:
                p.grad = self._delay_grad_views[i]
                if not all_none:
                    p.grad.zero_()
        if all_none:
            self._delay_grad_buffer.zero_()

    # ----------------------------------------------------------------------------- mixed precision
    def _setup_mixed_precision(self, module, mp):
        """T6i (``_MixedPrecision{param_dtype, reduce_dtype, buffer_dtype}``): fp32 parameters stay the
        autograd leaves (grads accumulate and are reduced from fp32 buckets, in ``reduce_dtype`` on
        the wire); each forward runs the module on ``param_dtype`` copies made by ONE multi-tensor
        cast launch, and backward casts the grads back in one launch."""
        self._mp_param_dtype = getattr(mp, "param_dtype", None) or torch.bfloat16
        buf_dt = getattr(mp, "buffer_dtype", None)
        if buf_dt is not None:
            for mod in module.modules():
                for n, b in list(mod._buffers.items()):
                    if b is not None and b.is_floating_point():
                        mod._buffers[n] = b.to(buf_dt)
        self._mp_names = [n for n, _ in module.named_parameters()]
        self._mp_params = [p for _, p in module.named_parameters()]

    def _mixed_precision_forward(self, inputs, kwargs):
        from torch.func import functional_call

        dt = self._mp_param_dtype
        casted = _CastParams.apply(dt, *self._mp_params)

        def cast(o):
            if isinstance(o, torch.Tensor):
                return o.to(dt) if o.is_floating_point() else o
            if isinstance(o, (list, tuple)):
                return type(o)(cast(x) for x in o)
            if isinstance(o, dict):
                return {k: cast(v) for k, v in o.items()}
            return o

        return functional_call(self.module, dict(zip(self._mp_names, casted)), tuple(cast(inputs)), cast(kwargs),
                               tie_weights=True, strict=False)

    # ----------------------------------------------------------------------------- setup
    @staticmethod
    def _group_from_mesh(device_mesh):
        """A 1-D device mesh names the data-parallel group (reference ``:688-717``)."""
        if getattr(device_mesh, "ndim", 1) != 1:
            raise RuntimeError("Only 1D device mesh is supported, but got {}.".format(device_mesh))
        get = getattr(device_mesh, "get_group", None)
        if get is None:
            raise TypeError("device_mesh must provide get_group() (a torch DeviceMesh or an xddp mesh)")
        try:
            return get(mesh_dim=0)
        except TypeError:
            return get()

    @staticmethod
    def _resolve_process_group(process_group):
        """xddp group, or a torch.distributed group (wrapped), or the default of either."""
        if process_group is not None and not isinstance(process_group, xdist.ProcessGroup):
            from ..distributed.torch_adapter import from_torch_process_group

            return from_torch_process_group(process_group)
        if process_group is not None:
            return process_group
        if xdist.is_initialized():
            return xdist.get_default_group()
        import torch.distributed as tdist

        if tdist.is_available() and tdist.is_initialized():
            from ..distributed.torch_adapter import from_torch_process_group

            return from_torch_process_group(None)
        return xdist.get_default_group()  # raises the "not initialized" error

    def _expect_sparse_gradient(self) -> List[bool]:
        """Parameters of ``nn.Embedding/EmbeddingBag(sparse=True)`` produce sparse gradients
        (reference ``_build_params_for_reducer``, ``pt:nn/parallel/distributed.py:1337-1346``)."""
        sparse_ids = set()
        for m in self.module.modules():
            if isinstance(m, (nn.Embedding, nn.EmbeddingBag)) and getattr(m, "sparse", False):
                sparse_ids.add(id(m.weight))
        return [id(p) in sparse_ids for p in self._module_parameters]

    def _build_reducer(self):
        C = load()
        params = self._module_parameters
        expect_sparse = self._expect_sparse_gradient()
        if any(expect_sparse) and self.gradient_as_bucket_view:
            logger.warning("xddp: sparse-gradient parameters do not live in buckets (gradient_as_bucket_view "
                           "applies to the dense ones)")
        if self.find_unused_parameters:
            limits = [self.first_bucket_bytes_cap, self.bucket_bytes_cap]
        else:
            limits = [sys.maxsize]
        idx, lims = C.compute_bucket_assignment_by_size(params, limits, expect_sparse)
        idx, lims = list(reversed(idx)), list(reversed(lims))
        cd = "" if self._comm_dtype is None else str(self._comm_dtype).replace("torch.", "")
        self._grad_target_views = None  # (bucket views of the previous reducer, if any)
        self.reducer = C.Reducer(
            params, idx, lims, self.process_group.comm,
            find_unused_parameters=self.find_unused_parameters,
            gradient_as_bucket_view=self.gradient_as_bucket_view,
            static_graph=False,
            bucket_bytes_cap=self.bucket_bytes_cap,
            first_bucket_bytes_cap=self.first_bucket_bytes_cap,
            comm_dtype=cd,
            param_names=self._param_names,
            skip_all_reduce_unused_params=self.skip_all_reduce_unused_params,
            tail_bucket_bytes_cap=self.bucket_plan.tail_bytes,
            expect_sparse=expect_sparse,
        )

    def _rebind_grad_accumulators(self, stream=None):
        """Re-create the AccumulateGrad nodes the Reducer hooks on under ``stream``.

        Autograd runs an AccumulateGrad node on the stream current when the node was created —
        for DDP that is the stream at construction time. A step captured into a HIP graph on a
        side stream must not touch another stream, so the graph helper rebinds the nodes to the
        capture stream first (call with no live autograd graph referencing the parameters)."""
        import gc

        gc.collect()
        if stream is None or self.device_type != "cuda":
            self.reducer.reinstall_hooks()
            return
        with torch.cuda.stream(stream):
            self.reducer.reinstall_hooks()

    def _sync_module_states(self, src: int = 0):
        C = load()
        tensors = [p.detach() for p in self.module.parameters()] + [b for b in self._buffers_list]
        tensors = [t for t in tensors if t.numel() > 0]
        if tensors:
            with torch.no_grad():
                C.broadcast_coalesced(self.process_group.comm, tensors, self.broadcast_bucket_size, src)

    # ----------------------------------------------------------------------------- forward
    def _pre_forward(self, *inputs, **kwargs):
        self._forward_count = getattr(self, "_forward_count", 0) + 1
        _fault.maybe_fail(self.process_group.rank(), self._forward_count)
        if self._delay_all_reduce_all_params or getattr(self, "_use_python_reducer", False):
            if self.device_ids:
                inputs = _to_device(inputs, self.device_ids[0])
                kwargs = _to_device(kwargs, self.device_ids[0])
            return inputs, kwargs
        if torch.is_grad_enabled() and self.require_backward_grad_sync:
            self.reducer.prepare_for_forward()
        work = Join.notify_join_context(self)
        if work is not None and not self._divide_by_initial_world_size:
            work.wait()
            self.reducer.set_gradient_divide_factor(float(work._ones.item()))
        rebuilt = torch.is_grad_enabled() and self.reducer.rebuild_buckets()
        if rebuilt:
            logger.info("xddp: rebuilt buckets: %s", self.reducer.bucket_sizes_bytes())
        if torch.is_grad_enabled() and self.gradient_as_bucket_view and self.device_type == "cuda" and \
                self._comm_dtype is None and os.environ.get("XDDP_GRAD_TARGETS", "1") != "0":
            # the library / multi-input linears write their weight gradients straight into these
            # bucket views (ops/linear.py set_grad_targets): no per-step copy into the buckets. A
            # registration is claimed by one backward, so it is renewed every forward; the views
            # themselves only change when the buckets are rebuilt.
            if rebuilt or getattr(self, "_grad_target_views", None) is None:
                _linear_ops.clear_grad_targets(self._module_parameters)  # views of the old layout
                self._grad_target_views = self.reducer.param_bucket_views()
            _linear_ops.set_grad_targets(self._module_parameters, self._grad_target_views)
        if self._check_sync_bufs_pre_fwd():
            self._sync_buffers()
        n = getattr(self, "_check_replicas_every", 0)
        if n > 0 and self._forward_count % n == 0 and torch.is_grad_enabled():
            rep = self.check_replicas(max_diff=False)
            if not rep["replicas_identical"]:
                raise RuntimeError(f"xddp DDP: model replicas diverged before forward {self._forward_count}: ranks "
                                   f"{rep['mismatch_ranks']} disagree with the majority (XDDP_CHECK_REPLICAS)")
        if self._join_config.enable:
            # tell joined ranks whether this iteration's backward syncs (their shadow collectives)
            self._check_global_requires_backward_grad_sync(is_joined_rank=False)
        if self.device_ids:
            inputs = _to_device(inputs, self.device_ids[0])
            kwargs = _to_device(kwargs, self.device_ids[0])
        return inputs, kwargs

    def check_replicas(self, max_diff: bool = True) -> dict:
        """Collective: compare every parameter (and, when buffers are broadcast every forward, every
        buffer) across the ranks of this DDP's group by one native checksum pass per rank
        (``utils/replicas.py``). Returns ``{"replicas_identical", "mismatch_ranks", "max_abs_diff",
        "checksum"}``. Buffers take local updates inside a forward (BatchNorm running stats) and are
        re-synced from rank 0 at the next one, so call this right after a buffer sync (as the
        per-forward check does) or pass through :meth:`_sync_buffers` first."""
        tensors = list(self._module_parameters)
        if self.will_sync_module_buffers():
            tensors += [b for b in self._buffers_list if b.numel() > 0]
        with torch.no_grad():
            return _replicas.check_replicas(tensors, self.process_group, max_diff=max_diff)

    def _check_global_requires_backward_grad_sync(self, is_joined_rank: bool):
        flag = not is_joined_rank and torch.is_grad_enabled() and self.require_backward_grad_sync
        t = torch.full((1,), 1 if flag else 0, dtype=torch.int32, device=self._comm_device)
        work = self.process_group.allreduce(t, xdist.ReduceOp.SUM)
        if is_joined_rank:
            work.wait()
            return bool(t.item() != 0)
        return work

    def _post_forward(self, output):
        self._clear_grad_buffer()
        if self._delay_all_reduce_all_params or getattr(self, "_use_python_reducer", False):
            return output
        if self._check_sync_bufs_post_fwd():
            self._sync_buffers()
        if torch.is_grad_enabled() and self.require_backward_grad_sync:
            self.require_forward_param_sync = True
            outs = _find_tensors(output) if (self.find_unused_parameters and not self.static_graph) else []
            self.reducer.prepare_for_backward(outs)
        else:
            self.require_forward_param_sync = False
        return output

    def forward(self, *inputs, **kwargs):
        with record_function("DistributedDataParallel.forward"):
            inputs, kwargs = self._pre_forward(*inputs, **kwargs)
            if self.mixed_precision is not None and torch.is_grad_enabled():
                output = self._mixed_precision_forward(inputs, kwargs)
            else:
                output = self.module(*inputs, **kwargs)
            return self._post_forward(output)

    # ----------------------------------------------------------------------------- buffers
    def will_sync_module_buffers(self) -> bool:
        return self.require_forward_param_sync and self.broadcast_buffers and len(self._buffers_list) > 0

    def _check_sync_bufs_pre_fwd(self) -> bool:
        hook = getattr(self, "buffer_hook", None)
        return self.will_sync_module_buffers() and (hook is None or hook[2] == BufferCommHookLocation.PRE_FORWARD)

    def _check_sync_bufs_post_fwd(self) -> bool:
        hook = getattr(self, "buffer_hook", None)
        return self.will_sync_module_buffers() and hook is not None and hook[2] == BufferCommHookLocation.POST_FORWARD

    def _register_buffer_comm_hook(self, state, hook: Callable,
                                   comm_hook_location=BufferCommHookLocation.POST_FORWARD):
        """Replace the per-forward rank-0 buffer broadcast with ``hook(state, {name: buffer})``
        (reference ``pt:nn/parallel/distributed.py:1909-1951``). The hook may return a list of
        futures; they are awaited at the end of the next backward (finalize), so e.g. an
        all-reduce of BN statistics overlaps the whole backward pass."""
        if not callable(hook):
            raise TypeError("buffer comm hook must be callable")
        self.buffer_hook = (hook, state, comm_hook_location)

    @property
    def named_module_buffers(self):
        return {n: b for n, b in self.module.named_buffers() if n not in self._params_and_buffers_to_ignore}

    def _find_common_rank(self, input_rank: int, rank_cond: bool) -> int:
        t = torch.tensor([input_rank if rank_cond else -1], device=self._comm_device)
        self.process_group.allreduce(t, xdist.ReduceOp.MAX).wait()
        r = int(t.item())
        if r == -1:
            raise ValueError("BUG! Expected rank_cond to be true for at least one process.")
        return r

    def _sync_buffers(self, src: int = 0, joined: bool = False):
        """Per-forward buffer sync: the registered buffer comm hook, or a coalesced broadcast from
        ``src`` (under Join: from a rank still training). ``joined=True`` is the shadow a joined
        rank runs in ``_DDPJoinHook.main_hook`` — the same collectives in the same order."""
        with torch.no_grad():
            if self._join_config.enable or joined:
                src = self._find_common_rank(self.process_group.rank(), not joined)
            hook = getattr(self, "buffer_hook", None)
            if hook is not None:
                futs = hook[0](hook[1], self.named_module_buffers)
                if futs:
                    if not joined and torch.is_grad_enabled() and self.require_backward_grad_sync:
                        self.reducer.install_post_backward_futures(list(futs))
                    else:
                        for f in futs:
                            f.wait()
                return
            C = load()
            bufs = [b for b in self._buffers_list if b.numel() > 0]
            if bufs:
                C.broadcast_coalesced(self.process_group.comm, bufs, self.broadcast_bucket_size, src)

    def _check_and_sync_module_buffers(self):
        if self.will_sync_module_buffers():
            self._sync_buffers(joined=True)

    def _sync_final_model(self, is_last_joiner: bool):
        src = self._find_common_rank(self.process_group.rank(), is_last_joiner)
        self._sync_module_states(src=src)

    # ----------------------------------------------------------------------------- no_sync / join
    @contextmanager
    def no_sync(self):
        """Accumulate grads locally; the first backward after the context reduces them."""
        old = self.require_backward_grad_sync
        self.require_backward_grad_sync = False
        try:
            yield
        finally:
            self.require_backward_grad_sync = old

    def join(self, divide_by_initial_world_size: bool = True, enable: bool = True,
             throw_on_early_termination: bool = False):
        return Join([self], enable, throw_on_early_termination,
                    divide_by_initial_world_size=divide_by_initial_world_size)

    def join_hook(self, **kwargs):
        return _DDPJoinHook(self, kwargs.get("divide_by_initial_world_size", True))

    @property
    def join_device(self):
        return self._comm_device

    @property
    def join_process_group(self):
        return self.process_group

    # ----------------------------------------------------------------------------- hooks
    def register_comm_hook(self, state: object, hook: Callable):
        """Register ``hook(state, bucket) -> Future[Tensor]`` (reference: ``:1953-2032``)."""
        if not callable(hook):
            raise TypeError("comm hook must be callable")
        self._comm_hooks.append((state, hook))
        if not getattr(self, "_use_python_reducer", False):  # python reducer: hook(state, (grad, param))
            self.reducer.register_comm_hook(state, hook)

    def _register_builtin_comm_hook(self, comm_hook_type):
        """Native builtin hooks: ALLREDUCE (default) or FP16/BF16 compression (fused casts)."""
        if comm_hook_type in (BuiltinCommHookType.FP16_COMPRESS, "FP16_COMPRESS"):
            self.reducer.set_comm_dtype("float16")
        elif comm_hook_type in (BuiltinCommHookType.BF16_COMPRESS, "BF16_COMPRESS"):
            self.reducer.set_comm_dtype("bfloat16")
        elif comm_hook_type in (BuiltinCommHookType.ALLREDUCE, "ALLREDUCE"):
            pass
        else:
            raise ValueError(f"unknown builtin comm hook {comm_hook_type}")

    def register_overlapped_optimizer(self, optimizer, schedule: str = "tail",
                                      tail_chunk_bytes: Optional[int] = None):
        """Run the optimizer update inside backward, bucket by bucket, on a side HIP stream; the
        compute stream waits for the side stream at the end of backward. Do not call
        ``optimizer.step()`` afterwards (the reference's ``_register_fused_optim`` contract,
        ``pt:nn/parallel/distributed.py:2061-2131``). Needs an optimizer with ``step_params``; the
        tail schedule also needs ``advance`` / ``step_slices`` (``FusedAdamW``, ``FusedAdam``), which
        the layer-wise ``FusedLAMB`` / ``FusedLARS`` cannot have (``schedule="backward"`` only).

        ``schedule="tail"`` (default) puts the updates where the GPU is otherwise idle — under the
        LAST bucket's all-reduce, which nothing in backward can hide:

        * every other bucket's all-reduce is launched as usual when the bucket is ready, but its
          update is deferred;
        * the last bucket is all-reduced in chunks of ``tail_chunk_bytes`` (default
          ``XDDP_TAIL_CHUNK_MB`` = 64 MiB; Llama-3-8B's 1.05 GB token-embedding gradient, which is
          ready last and forms the tail alone, becomes 16 collectives);
        * right after those launches the side stream runs the deferred updates (each after its own
          bucket's collective), then the tail's chunk i update after chunk i's collective — so the
          tail all-reduce runs concurrently with optimizer work the step has to do anyway, and at
          most one chunk's update is left after the last chunk's collective.

        ``schedule="backward"`` updates each bucket as soon as its own all-reduce is done, so the
        (HBM-bound) updates overlap the remaining backward kernels instead; on one MI355X that
        measured no gain (hipBLASLt's backward GEMMs already occupy every CU) and it leaves the
        tail all-reduce exposed.
        """
        if schedule not in ("tail", "backward"):
            raise ValueError(f"unknown overlapped-optimizer schedule {schedule!r} (use 'tail' or 'backward')")
        name = type(optimizer).__name__
        if not hasattr(optimizer, "step_params"):
            raise TypeError(f"register_overlapped_optimizer needs an optimizer with step_params (FusedAdamW, "
                            f"FusedAdam, FusedLAMB, FusedLARS); {name} has none")
        if schedule == "tail":
            for attr in ("advance", "step_slices"):
                if not hasattr(optimizer, attr):
                    raise TypeError(
                        f"register_overlapped_optimizer(schedule='tail') updates the last bucket chunk by chunk and "
                        f"needs an optimizer with {attr} (FusedAdamW, FusedAdam); {name} has none. A layer-wise "
                        f"optimizer (FusedLAMB, FusedLARS) needs a whole tensor's norm before it can update any "
                        f"element of it: use schedule='backward', which steps whole parameters bucket by bucket")
        if tail_chunk_bytes is None:
            tail_chunk_bytes = int(float(os.environ.get("XDDP_TAIL_CHUNK_MB", "64")) * (1 << 20))
        side = torch.cuda.Stream(self._param_device) if self.device_type == "cuda" else None
        state = {"opt": optimizer, "side": side, "queued": False, "ddp": weakref.ref(self), "deferred": [],
                 "schedule": schedule, "chunk_bytes": max(1 << 16, int(tail_chunk_bytes)), "last_chunks": 0,
                 "pairs": []}
        self._overlap_state = state

        def run_side(fn):
            if side is None:
                fn()
                return
            # the side stream starts after everything the compute stream has enqueued (this
            # bucket's gradients), then each update waits for its own collective
            side.wait_stream(torch.cuda.current_stream(side.device))
            with torch.cuda.stream(side):
                fn()

        def flush_deferred():
            pending, state["deferred"] = state["deferred"], []
            for work, ps, gs in pending:
                work.wait()
                optimizer.step_params(ps, gs)

        def join():
            state["queued"] = False
            if state["deferred"]:  # the last bucket never reached the hook (e.g. skipped as unused)
                run_side(flush_deferred)
            if side is not None:
                torch.cuda.current_stream(side.device).wait_stream(side)
            # The hook hands the reducer an already-completed future (the collectives are still in
            # flight on the comm stream), so without bucket views the reducer's own copy of the
            # bucket into .grad may read the buffer before the all-reduce lands: copy the reduced
            # bucket views into .grad again, ordered after the side stream (which waited for every
            # collective).
            pairs, state["pairs"] = state["pairs"], []
            with torch.no_grad():
                for p, g in pairs:
                    if p.grad is not None and p.grad.data_ptr() != g.data_ptr():
                        p.grad.copy_(g.view_as(p.grad) if g.shape != p.grad.shape else g)

        def done(buf):
            fut = torch.futures.Future()
            fut.set_result(buf)
            return fut

        def hook(st, bucket):
            ddp = st["ddp"]()
            pg = ddp.process_group
            buf = bucket.buffer()
            if not st["queued"]:
                st["queued"] = True
                torch.autograd.Variable._execution_engine.queue_callback(join)
            if not ddp.gradient_as_bucket_view:
                st["pairs"].extend(zip(bucket.parameters(), bucket.gradients()))
            if st["schedule"] == "backward":
                work = pg.allreduce(buf, xdist.ReduceOp.AVG)
                st["deferred"].append((work, bucket.parameters(), bucket.gradients()))
                run_side(flush_deferred)
                return done(buf)
            if not bucket.is_last():
                st["deferred"].append((pg.allreduce(buf, xdist.ReduceOp.AVG), bucket.parameters(),
                                       bucket.gradients()))
                return done(buf)
            chunks = tail_chunks(buf.numel(), buf.element_size(), st["chunk_bytes"])
            works = [pg.allreduce(buf[lo:hi], xdist.ReduceOp.AVG) for lo, hi in chunks]
            st["last_chunks"] = len(chunks)
            params, grads = bucket.parameters(), bucket.gradients()
            spans = list(zip(bucket.offsets(), bucket.lengths()))
            optimizer.advance(params)

            def updates():
                flush_deferred()
                for (lo, hi), work in zip(chunks, works):
                    work.wait()
                    pieces = [(p, g, max(lo, o) - o, min(hi, o + n) - o)
                              for p, g, (o, n) in zip(params, grads, spans) if max(lo, o) < min(hi, o + n)]
                    optimizer.step_slices(pieces)

            run_side(updates)
            return done(buf)

        self.register_comm_hook(state, hook)

    def _register_fused_optim(self, optim_cls, *args, optim_params=None, **kwargs):
        from .comm_hooks.optimizer_overlap_hooks import _OptimizerHookState, _hook_then_optimizer
        from .comm_hooks.default_hooks import allreduce_hook

        state = _OptimizerHookState(optim_cls, self._module_parameters if optim_params is None else optim_params,
                                    *args, **kwargs)
        self.register_comm_hook(self.process_group, _hook_then_optimizer(allreduce_hook, state))

    # ----------------------------------------------------------------------------- misc
    def _set_static_graph(self):
        if self.static_graph:
            return
        self.static_graph = True
        self.reducer.set_static_graph()

    def _get_ddp_logging_data(self) -> dict:
        d = dict(self.reducer.construction_data())
        d["bucket_policy"] = self.bucket_plan.policy
        for k, v in self.reducer.runtime_stats().items():
            v = float(v)
            # NaN = never measured (e.g. comm fields when no collective crossed a link)
            d[k] = None if v != v else (int(v) if v.is_integer() else v)
        d["bucket_comm_times"] = [round(t) for t in self.reducer.bucket_comm_times()]
        d["module_name"] = type(self.module).__name__
        d["device_ids"] = "" if not self.device_ids else ", ".join(str(x.index) for x in self.device_ids)
        d["broadcast_buffers"] = int(self.broadcast_buffers)
        d["is_multi_device_module"] = 0
        d["num_parameter_tensors"] = len(self._module_parameters)
        d["total_parameter_size_bytes"] = sum(p.numel() * p.element_size() for p in self._module_parameters)
        d["dtypes"] = ", ".join(sorted({str(p.dtype).replace("torch.", "") for p in self._module_parameters}))
        d["comm_hook"] = "" if not self._comm_hooks else getattr(self._comm_hooks[0][1], "__qualname__", "hook")
        return d

    def _set_ddp_runtime_logging_sample_rate(self, sample_rate: int):
        if sample_rate < 1:
            raise ValueError("DDP runtime logging sample rate should be equal or greater than 1")
        self.reducer.set_runtime_logging_sample_rate(sample_rate)

    def _get_ddp_bucket_indices(self):
        return self.reducer.bucket_indices()

    def _remove_autograd_hooks(self):
        self.reducer.remove_autograd_hooks()
        _linear_ops.clear_grad_targets(self._module_parameters)  # no weight gradient into our buckets
        self._grad_target_views = None
        for h in self._accum_grad_hooks:
            h.remove()
        self._accum_grad_hooks = []

    def _check_reducer_finalized(self):
        self.reducer.check_finalized()

    def _update_process_group(self, new_process_group):
        """Continue training on a new (shrunk/expanded) group without rebuilding the wrapper."""
        self.process_group = new_process_group
        self.reducer.set_comm(new_process_group.comm)

    def __getstate__(self):
        self._check_default_group()
        attrs = copy.copy(self.__dict__)
        del attrs["process_group"]
        del attrs["reducer"]
        attrs.pop("_grad_target_views", None)  # views into this process's buckets
        attrs["_comm_hooks"] = []
        attrs["_accum_grad_hooks"] = []
        return attrs

    def __setstate__(self, state):
        self.process_group = self._resolve_process_group(None)
        super().__setstate__(state)
        self.__dict__.setdefault("require_forward_param_sync", True)
        self.__dict__.setdefault("require_backward_grad_sync", True)
        self._build_reducer()
        if self.static_graph:
            self.static_graph = False
            self._set_static_graph()
        if self.__dict__.get("_use_python_reducer", False):
            self._register_accum_grad_hook()

    def _check_default_group(self):
        if xdist.is_initialized() and self.process_group is not xdist.get_default_group():
            raise RuntimeError("DDP pickling/unpickling are only supported when using DDP with the default process "
                               "group.")


DDP = DistributedDataParallel
