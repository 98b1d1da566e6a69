"""Fused multi-tensor optimizers and grad-norm clipping on HIP kernels.

Reference hot path: ``optim.SGD`` → one ``_foreach_add_`` over all
params. Here one native launch per (dtype-group × 40 tensors) does the full update —
weight decay, momentum/Nesterov, Adam moments, bias correction, and optionally fp32
master weights for bf16/fp16 models — reading each operand once with 16-byte loads.
``grad_scale`` (a device scalar) lets a clip coefficient or loss-scale be applied inside
the same pass without a host sync.

CPU tensors take an equivalent torch reference path (the GPU-free test backend).
"""
from __future__ import annotations

import functools
from collections import defaultdict
from typing import Iterable, List, Optional

import torch
from torch.optim import Optimizer

from .._native import load

__all__ = ["FusedSGD", "FusedAdamW", "FusedAdam", "clip_grad_norm_", "grad_norm", "stochastic_round_bf16"]


def _group_key(p: torch.Tensor, g: torch.Tensor):
    return (p.device, p.dtype, g.dtype)


def _dense_like(p: torch.Tensor) -> torch.Tensor:
    return torch.empty_strided(p.size(), p.stride(), dtype=torch.float32, device=p.device)


def _flat_range(t: torch.Tensor, lo: int, hi: int) -> torch.Tensor:
    """Elements [lo, hi) of a dense (possibly permuted-stride) tensor in memory order, as a 1-D view."""
    expect = 1
    for st, sz in sorted((st, sz) for st, sz in zip(t.stride(), t.size()) if sz != 1):
        if st != expect:
            raise ValueError("slice updates need dense parameters / gradients / states")
        expect *= sz
    return t.as_strided((hi - lo,), (1,), t.storage_offset() + lo)


_QGROUP = 128      # elements per scale of the 8-bit optimizer states
_E4M3_MAX = 448.0
_FLT_MIN = 1.17549435e-38


@functools.lru_cache(maxsize=None)
def _e4m3_table(device) -> torch.Tensor:
    """Value of every OCP e4m3 code (256 entries, built in software; 0x7f / 0xff are NaN). The
    first 127 entries are the non-negative grid in ascending order, so a code is its own index."""
    vals = []
    for code in range(128):
        e, m = code >> 3, code & 7
        vals.append(m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
    vals[127] = float("nan")
    return torch.tensor(vals + [-v for v in vals], dtype=torch.float32, device=device)


def _mix64(z: int) -> int:  # splitmix64 finalizer
    z &= (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & ((1 << 64) - 1)
    return z ^ (z >> 31)


def _group_expand(scale: torch.Tensor, n: int) -> torch.Tensor:
    return scale.repeat_interleave(_QGROUP)[:n]


def _dequantize_e4m3(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return _e4m3_table(codes.device)[codes.long()] * _group_expand(scale, codes.numel())


def _quantize_e4m3_sr(x: torch.Tensor, u: torch.Tensor, nonneg: bool):
    """Block-scaled e4m3 codes of the 1-D fp32 ``x`` (which starts at a group boundary), rounded
    stochastically with the uniform [0, 1) numbers ``u``: (uint8 codes, fp32 scale per group)."""
    n = x.numel()
    ng = (n + _QGROUP - 1) // _QGROUP
    ax = x.abs()
    amax = torch.nn.functional.pad(ax, (0, ng * _QGROUP - n)).view(ng, _QGROUP).amax(1)
    scale = amax / _E4M3_MAX
    inv = torch.where(scale >= _FLT_MIN, 1.0 / scale, torch.zeros_like(scale))
    q = (ax * _group_expand(inv, n)).clamp_(max=_E4M3_MAX)
    grid = _e4m3_table(x.device)[:127]
    idx = torch.searchsorted(grid, q, right=True) - 1  # grid[idx] <= q < grid[idx + 1]
    lo, hi = grid[idx], grid[(idx + 1).clamp_(max=126)]
    up = torch.where(hi > lo, (q - lo) / (hi - lo), torch.zeros_like(q))
    code = idx + (u < up)
    if nonneg:  # a live element never gets code 0
        code = torch.where((x > 0) & (code == 0), torch.ones_like(code), code)
    else:
        code = code + 128 * torch.signbit(x)
    return code.to(torch.uint8), scale


_M32 = 0xFFFFFFFF


def _sr_param_key(seed: int, ordinal: int, step: int) -> int:
    """``kp``, the hash key of the stochastically rounded parameter write: a third stream next to the
    8-bit moments' ``km`` / ``ks`` (the low / high half of ``key``), the splitmix64 output after it."""
    key = _mix64(seed ^ _mix64((ordinal << 32) | step))
    return _mix64(key + 0x9E3779B97F4A7C15) & _M32


def _mul32(x: torch.Tensor, c: int) -> torch.Tensor:
    """``x * c mod 2^32`` for an int64 tensor of 32-bit values, without overflowing int64."""
    return ((((x * (c >> 16)) & 0xFFFF) << 16) + x * (c & 0xFFFF)) & _M32


def _mix32(x: torch.Tensor) -> torch.Tensor:  # the kernels' mix32, on 32-bit values held in int64
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


@torch.no_grad()
def stochastic_round_bf16(x: torch.Tensor, seed: int, ordinal: int = 0, step: int = 0, offset: int = 0) -> torch.Tensor:
    """The fp32 tensor ``x`` (dense, taken in memory order) rounded stochastically to bf16.

    Element ``i`` with bits ``u`` gets the upper 16 bits of ``u + r``, ``r`` being 16 random bits: the
    value is rounded away from zero with probability (discarded 16 bits) / 65536 and truncated
    otherwise, so the result is ``x`` in expectation, and a value that already is a bf16 is
    returned unchanged. A finite value never becomes inf (where the sum's exponent would be all ones
    the upper 16 bits of ``u`` are kept: the largest finite bf16 of that sign), +-inf stay, and NaN
    gives the quiet NaN ``0x7FC0``. ``r`` is the top half of ``mix32(lo ^ kp ^ hi)`` for the element
    index ``e = offset + i`` (``lo = e mod 2^32``, ``hi = (e >> 32) * 0x9e3779b9 mod 2^32``) and
    ``kp`` the parameter-write key of (``seed``, ``ordinal``, ``step``): the third stream of the hash
    that rounds the 8-bit optimizer states. CUDA tensors run the HIP kernel, CPU tensors the same
    integer arithmetic in torch; the two agree bit for bit.
    """
    if x.dtype != torch.float32:
        raise TypeError(f"stochastic_round_bf16 expects a float32 tensor, got {x.dtype}")
    seed, ordinal, step, offset = int(seed), int(ordinal), int(step), int(offset)
    if not (0 <= seed < 1 << 63 and 0 <= ordinal < 1 << 32 and 0 <= step < 1 << 32 and 0 <= offset < 1 << 62):
        raise ValueError("stochastic_round_bf16: seed in [0, 2^63), ordinal and step in [0, 2^32), offset >= 0")
    n = x.numel()
    src = _flat_range(x, 0, n)  # (raises for a tensor that is not dense)
    out = torch.empty_like(x, dtype=torch.bfloat16)  # the same strides
    if n == 0:
        return out
    if x.device.type == "cuda":
        load().stochastic_round_bf16(x, out, seed, ordinal, step, offset)
        return out
    u = src.contiguous().view(torch.int32).to(torch.int64) & _M32
    e = torch.arange(offset, offset + n, dtype=torch.int64)
    hi = ((e >> 32) * 0x9E3779B9) & _M32
    r = _mix32((e & _M32) ^ _sr_param_key(seed, ordinal, step) ^ hi) >> 16
    t = (u + r) & _M32
    t = torch.where((t & 0x7F800000) == 0x7F800000, u, t)  # no overflow to inf; +-inf keep their bits
    t = torch.where(((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0), torch.full_like(t, 0x7FC00000), t)
    bits = t >> 16
    bits = (bits - ((bits & 0x8000) << 1)).to(torch.int16)
    _flat_range(out, 0, n).copy_(bits.view(torch.bfloat16))
    return out


class _KeepStateDtypes:
    """``load_state_dict`` that keeps every state tensor's saved dtype. torch's casts each of them
    to the parameter's dtype, which for a bf16 model rounds the fp32 moments, momentum buffers and
    master weights to bf16 (the fused kernels then reject them) and would turn the 8-bit states'
    uint8 codes and fp32 scales into bf16. State tensors only move to the parameter's device."""

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        saved_ids = [k for g in state_dict["param_groups"] for k in g["params"]]
        params = [p for g in self.param_groups for p in g["params"]]
        for k, p in zip(saved_ids, params):
            for key, val in state_dict["state"].get(k, {}).items():
                if isinstance(val, torch.Tensor) and key != "step":
                    self.state[p][key] = val.to(device=p.device)
        for g in self.param_groups:
            for key, val in self.defaults.items():
                g.setdefault(key, val)  # a checkpoint from before an option existed
        for cache in ("_group_of", "_ordinal_of"):
            self.__dict__.pop(cache, None)


class FusedSGD(_KeepStateDtypes, Optimizer):
    """SGD with momentum/dampening/Nesterov/weight decay (torch.optim.SGD semantics).

    ``master_weights=True`` keeps fp32 master copies for low-precision params.
    """

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, maximize: bool = False,
                 master_weights: bool = False):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                        nesterov=nesterov, maximize=maximize, master_weights=master_weights)
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure=None, grad_scale: Optional[torch.Tensor] = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        C = load()
        for group in self.param_groups:
            buckets = defaultdict(lambda: ([], [], [], []))
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                first = "momentum_buffer" not in st
                if group["momentum"] != 0 and first:
                    st["momentum_buffer"] = _dense_like(p)
                use_master = group["master_weights"] and p.dtype in (torch.bfloat16, torch.float16)
                if use_master and "master" not in st:
                    st["master"] = p.detach().float().clone(memory_format=torch.preserve_format)
                key = _group_key(p, p.grad) + (first, use_master)
                b = buckets[key]
                b[0].append(st["master"] if use_master else p)
                b[1].append(p.grad)
                b[2].append(st.get("momentum_buffer"))
                b[3].append(p)
            for (dev, pdt, gdt, first, use_master), (ps, gs, bufs, orig) in buckets.items():
                mom = group["momentum"]
                bufs = bufs if mom != 0 else []
                if dev.type == "cuda" and use_master:  # one pass: update fp32 masters, round into the params
                    C.fused_sgd_master(ps, gs, bufs, orig, group["lr"], mom, group["dampening"],
                                       group["weight_decay"], group["nesterov"], group["maximize"], first, grad_scale)
                elif dev.type == "cuda":
                    C.fused_sgd(ps, gs, bufs, group["lr"], mom, group["dampening"], group["weight_decay"],
                                group["nesterov"], group["maximize"], first, grad_scale)
                else:
                    self._cpu_step(ps, gs, bufs, group, first, grad_scale)
                    if use_master:
                        for m, p in zip(ps, orig):
                            p.copy_(m)
        return loss

    @staticmethod
    def _cpu_step(ps, gs, bufs, group, first, grad_scale):
        lr, mom, damp, wd = group["lr"], group["momentum"], group["dampening"], group["weight_decay"]
        for i, (p, g) in enumerate(zip(ps, gs)):
            d = g.float()
            if grad_scale is not None:
                d = d * grad_scale.float()
            if group["maximize"]:
                d = -d
            if wd != 0:
                d = d + wd * p.float()
            if mom != 0:
                buf = bufs[i]
                if first:
                    buf.copy_(d)
                else:
                    buf.mul_(mom).add_(d, alpha=1 - damp)
                d = d + mom * buf if group["nesterov"] else buf
            p.copy_(p.float() - lr * d)


class FusedAdamW(_KeepStateDtypes, Optimizer):
    """Adam / AdamW (decoupled weight decay), torch.optim semantics, no amsgrad.

    ``state_bits=32`` (default) keeps fp32 moments. ``state_bits=8`` keeps both moments as OCP e4m3
    codes with one fp32 scale per group of 128 consecutive elements of the parameter in memory order
    (the last group may be short): per parameter ``exp_avg_q`` / ``exp_avg_sq_q`` (uint8, ``numel``)
    and ``exp_avg_scale`` / ``exp_avg_sq_scale`` (fp32, ``ceil(numel / 128)``), 2.06 instead of 8
    bytes per parameter. A scale is its group's maximum / 448; the second moment is stored as
    ``sqrt(exp_avg_sq)``, and a non-zero root never gets code 0. Each step dequantises the moments,
    applies exactly the 32-bit update (the parameters and masters use the fresh fp32 moments) and
    re-quantises with stochastic rounding: round-to-nearest would drop every change of less than
    half a code step (a code step is 6.25 % of the value), so with ``beta2 = 0.999`` the second
    moment could never decay. The random bits are a stateless hash of (``seed``, the parameter's
    ordinal in the optimizer, its step, the element index, the moment): a run is reproducible, and
    independent of how parameters are grouped into launches or sliced. The CPU path draws its bits
    from a ``torch.Generator`` seeded from the same tuple, so it matches the GPU path in
    distribution, not bit for bit. :meth:`decode_states` gives the moments back in fp32.

    ``param_rounding="stochastic"`` (default ``"nearest"``) trains bf16 parameters without the fp32
    master copy: each is updated in fp32 from its bf16 value and written back with
    :func:`stochastic_round_bf16`, keyed by (``seed``, the parameter's ordinal, its step, the element
    index), so an update below half a bf16 ulp is applied in expectation where round-to-nearest
    would drop it every step. No ``master`` state exists (``master_weights=True`` is refused), fp32
    parameters of the same optimizer are updated as ever, fp16 ones are refused. It combines with
    either ``state_bits``; the CPU path rounds with the GPU's bits. Replicas that apply the same
    gradients with the same ``seed`` stay bitwise identical.

    With ``state_bits=8`` or ``param_rounding="stochastic"`` a step cannot be captured into a HIP
    graph (``RuntimeError``): the step count is a host value baked into the launch, and a replayed
    graph would round with the same random bits forever.
    """

    _decoupled = True

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 maximize: bool = False, master_weights: bool = False, amsgrad: bool = False, state_bits: int = 32,
                 seed: int = 0, param_rounding: str = "nearest"):
        if amsgrad:
            raise NotImplementedError("amsgrad is not supported by the fused kernel")
        if state_bits not in (8, 32):
            raise ValueError(f"state_bits must be 32 or 8, got {state_bits!r}")
        if not 0 <= int(seed) < 1 << 63:
            raise ValueError("seed must be in [0, 2^63)")
        if param_rounding not in ("nearest", "stochastic"):
            raise ValueError(f"param_rounding must be 'nearest' or 'stochastic', got {param_rounding!r}")
        if param_rounding == "stochastic" and master_weights:
            raise ValueError("param_rounding='stochastic' replaces the fp32 master weights: "
                             "master_weights must be False")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=maximize,
                        master_weights=master_weights, state_bits=state_bits, seed=int(seed),
                        param_rounding=param_rounding)
        super().__init__(params, defaults)
        self._slice_pos = {}  # 8-bit states: how far this step's pieces of a parameter have come
        for group in self.param_groups:
            for p in group["params"]:
                self._stochastic(p, group)  # (refuses fp16 parameters)

    @torch.no_grad()
    def step(self, closure=None, grad_scale: Optional[torch.Tensor] = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._refuse_capture()
        for group in self.param_groups:
            # create state and bump the step of every parameter with a gradient, then update whole parameters
            items = [(p, p.grad, 0, p.numel()) for p in group["params"] if p.grad is not None]
            for p, *_ in items:
                self._init_state(p, group)["step"] += 1
            (self._step8 if group["state_bits"] == 8 else self._step32)(group, items, grad_scale)
        return loss

    def _step32(self, group, ranges, grad_scale):
        """fp32 states: update ``ranges`` = ``[(param, grad, lo, hi)]`` with each parameter's current step
        count, one launch per (device, dtypes, step, master, rounding)."""
        b1, b2 = group["betas"]
        # params, grads, exp_avgs, exp_avg_sqs, masters, (ordinal, element offset) of a stochastically rounded range
        buckets = defaultdict(lambda: ([], [], [], [], [], []))
        for p, g, lo, hi in ranges:
            st = self.state[p]
            sr = self._stochastic(p, group)
            b = buckets[_group_key(p, g) + (st["step"], "master" in st, sr)]
            whole = lo == 0 and hi == p.numel()
            cut = (lambda t: t) if whole else (lambda t: _flat_range(t, lo, hi))
            b[0].append(cut(p))
            b[1].append(cut(g))
            b[2].append(cut(st["exp_avg"]))
            b[3].append(cut(st["exp_avg_sq"]))
            if "master" in st:
                b[4].append(cut(st["master"]))
            if sr:
                b[5].append((self._ordinal(p), lo))
        for (dev, pdt, gdt, step, has_master, sr), (ps, gs, m1, m2, masters, keys) in buckets.items():
            if dev.type != "cuda":
                self._cpu_step(ps, gs, m1, m2, masters, group, step, grad_scale, keys if sr else None)
            elif sr:
                load().fused_adam_sr(ps, gs, m1, m2, [o for o, _ in keys], [e for _, e in keys], group["lr"], b1, b2,
                                     group["eps"], group["weight_decay"], step, group["seed"], self._decoupled,
                                     group["maximize"], grad_scale)
            else:
                load().fused_adam(ps, gs, m1, m2, masters, group["lr"], b1, b2, group["eps"], group["weight_decay"],
                                  step, self._decoupled, group["maximize"], grad_scale)

    def _stochastic(self, p, group) -> bool:
        """Whether ``p`` is written with stochastic rounding (bf16 parameters of a
        ``param_rounding="stochastic"`` group; fp32 ones are exact as they are)."""
        if group.get("param_rounding", "nearest") != "stochastic" or p.dtype == torch.float32:
            return False
        if p.dtype != torch.bfloat16:
            raise ValueError(f"param_rounding='stochastic' supports bf16 (and fp32) parameters, got {p.dtype}")
        if group["master_weights"]:
            raise ValueError("param_rounding='stochastic' replaces the fp32 master weights: "
                             "master_weights must be False")
        return True

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """As the base class; ``param_rounding`` stays this optimizer's. A state saved with fp32 master
        weights loads into a ``param_rounding="stochastic"`` optimizer: every such parameter becomes
        ``stochastic_round_bf16(master)`` keyed at the saved step, and its master is dropped. A state
        saved with stochastic rounding has no masters to give a ``"nearest"`` optimizer: ``ValueError``."""
        own = [g["param_rounding"] for g in self.param_groups]
        saved = [g.get("param_rounding", "nearest") for g in state_dict["param_groups"]]
        if any(s == "stochastic" and o != "stochastic" for o, s in zip(own, saved)):
            raise ValueError("this state was saved with param_rounding='stochastic': it holds no fp32 master weights, "
                             "and its bf16 parameters carry the rounding. Load it into an optimizer constructed "
                             "with param_rounding='stochastic'")
        super().load_state_dict(state_dict)
        for group, rounding in zip(self.param_groups, own):
            group["param_rounding"] = rounding
            if rounding != "stochastic":
                continue
            group["master_weights"] = False
            for p in group["params"]:
                master = self.state[p].pop("master", None) if p in self.state else None
                if master is not None and self._stochastic(p, group):
                    p.copy_(stochastic_round_bf16(master, group["seed"], self._ordinal(p), self.state[p]["step"]))

    def _group_index(self, p):
        if not hasattr(self, "_group_of"):
            self._group_of = {id(q): gi for gi, grp in enumerate(self.param_groups) for q in grp["params"]}
        return self._group_of.get(id(p))

    def _ordinal(self, p):
        if not hasattr(self, "_ordinal_of"):
            self._ordinal_of = {id(q): i for i, q in enumerate(q for grp in self.param_groups for q in grp["params"])}
        return self._ordinal_of[id(p)]

    def _refuse_capture(self):
        if not (torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()):
            return
        if any(g["state_bits"] == 8 for g in self.param_groups):
            raise RuntimeError("FusedAdamW(state_bits=8) cannot be captured into a HIP graph: the step count that "
                               "seeds the stochastic rounding is a host value, so a replay would reuse one set of "
                               "random bits; step outside the capture, or use state_bits=32")
        if any(g.get("param_rounding") == "stochastic" for g in self.param_groups):
            raise RuntimeError("FusedAdamW(param_rounding='stochastic') cannot be captured into a HIP graph: the "
                               "step count that seeds the stochastic rounding is a host value, so a replay would "
                               "reuse one set of random bits; step outside the capture, or use "
                               "param_rounding='nearest'")

    def _init_state(self, p, group):
        st = self.state[p]
        if "step" in st:
            return st
        if group["state_bits"] == 8:
            _flat_range(p, 0, p.numel())  # (raises for a parameter that is not dense)
            ng = (p.numel() + _QGROUP - 1) // _QGROUP
        st["step"] = 0
        for name in ("exp_avg", "exp_avg_sq"):
            if group["state_bits"] == 8:
                st[name + "_q"] = torch.zeros(p.numel(), dtype=torch.uint8, device=p.device)
                st[name + "_scale"] = torch.zeros(ng, dtype=torch.float32, device=p.device)
            else:
                st[name] = _dense_like(p).zero_()
        if group["master_weights"] and p.dtype in (torch.bfloat16, torch.float16):
            st["master"] = p.detach().float().clone(memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step_params(self, params, grads):
        """Step only ``params`` with the given gradients (e.g. one DDP bucket's reduced views, from
        an overlapped-optimizer comm hook): same update as ``step`` for those parameters."""
        live = [(p, g) for p, g in zip(params, grads) if g is not None and self._group_index(p) is not None]
        self.advance([p for p, _ in live])
        self.step_slices([(p, g, 0, p.numel()) for p, g in live])

    @torch.no_grad()
    def advance(self, params):
        """Start this step for ``params`` (state created on first use, step count + 1) without
        updating them; :meth:`step_slices` then updates them piecewise with that step count."""
        self._refuse_capture()
        for p in params:
            gi = self._group_index(p)
            if gi is not None:
                self._init_state(p, self.param_groups[gi])["step"] += 1
                self._slice_pos[p] = 0

    @torch.no_grad()
    def step_slices(self, pieces):
        """Update element ranges of parameters: ``pieces`` = ``[(param, grad, lo, hi)]`` with
        ``[lo, hi)`` in memory order of the (dense) param; ``grad`` has the param's shape and
        strides. Uses each param's current step count (:meth:`advance` first). AdamW is elementwise,
        so updating a param in several slices is bitwise the same as updating it at once — the
        overlapped optimizer steps a chunked tail bucket this way, chunk by chunk as each chunk's
        all-reduce lands.

        With ``state_bits=8`` a group of 128 elements can only be re-quantised once its whole
        gradient is there, so within one step the pieces of a parameter must arrive in ascending,
        contiguous order (the first at 0, each next one where the last ended; anything else raises),
        and a piece ``[lo, hi)`` updates ``[lo // 128 * 128, hi // 128 * 128)``, or up to ``numel``
        when ``hi == numel``: every group is updated by the piece that delivers its last element.
        The result is still bitwise that of the whole-parameter update."""
        self._refuse_capture()
        per_group = defaultdict(list)
        for p, g, lo, hi in pieces:
            gi = self._group_index(p)
            if gi is not None and g is not None and hi > lo:
                per_group[gi].append((p, g, lo, hi))
        for gi, items in per_group.items():
            group = self.param_groups[gi]
            if group["state_bits"] == 8:
                ranges = []
                for p, g, lo, hi in items:
                    if self._init_state(p, group)["step"] == 0:
                        raise RuntimeError("step_slices before advance() for this step")
                    if lo != self._slice_pos.get(p, 0):
                        raise RuntimeError(f"state_bits=8: a parameter's pieces must arrive in ascending, contiguous "
                                           f"order within a step (expected one from {self._slice_pos.get(p, 0)}, got "
                                           f"[{lo}, {hi}))")
                    self._slice_pos[p] = hi
                    lo, hi = lo // _QGROUP * _QGROUP, hi if hi == p.numel() else hi // _QGROUP * _QGROUP
                    if hi > lo:
                        ranges.append((p, g, lo, hi))
                self._step8(group, ranges, None)
                continue
            for p, *_ in items:
                if self._init_state(p, group)["step"] == 0:
                    raise RuntimeError("step_slices before advance() for this step")
            self._step32(group, items, None)

    def _step8(self, group, ranges, grad_scale):
        """8-bit states: update ``ranges`` = ``[(param, grad, lo, hi)]``, ``lo`` a multiple of 128 and
        ``hi`` one too or the parameter's numel, with each parameter's current step count."""
        b1, b2 = group["betas"]
        buckets = defaultdict(lambda: tuple([] for _ in range(9)))
        for p, g, lo, hi in ranges:
            st = self.state[p]
            if g.stride() != p.stride() and not (g.is_contiguous() and p.is_contiguous()):
                raise ValueError("state_bits=8 needs the gradient in the parameter's memory order")
            b = buckets[_group_key(p, g) + (st["step"], "master" in st, self._stochastic(p, group))]
            glo, ghi = lo // _QGROUP, (hi + _QGROUP - 1) // _QGROUP
            b[0].append(_flat_range(p, lo, hi))
            b[1].append(_flat_range(g, lo, hi))
            b[2].append(st["exp_avg_q"][lo:hi])
            b[3].append(st["exp_avg_scale"][glo:ghi])
            b[4].append(st["exp_avg_sq_q"][lo:hi])
            b[5].append(st["exp_avg_sq_scale"][glo:ghi])
            if "master" in st:
                b[6].append(_flat_range(st["master"], lo, hi))
            b[7].append(self._ordinal(p))
            b[8].append((glo, p.numel()))
        for (dev, pdt, gdt, step, has_master, sr), (ps, gs, mq, ms, sq, ss, masters, ords, offs) in buckets.items():
            if dev.type == "cuda":
                load().fused_adam8(ps, gs, mq, ms, sq, ss, masters, ords, [o for o, _ in offs], group["lr"], b1, b2,
                                   group["eps"], group["weight_decay"], step, group["seed"], self._decoupled,
                                   group["maximize"], grad_scale, stochastic_params=sr)
                continue
            for i, (p, g) in enumerate(zip(ps, gs)):
                n, (glo, numel) = p.numel(), offs[i]
                m = _dequantize_e4m3(mq[i], ms[i])
                v = _dequantize_e4m3(sq[i], ss[i]).square_()
                self._cpu_step([p], [g], [m], [v], masters[i:i + 1], group, step, grad_scale,
                               [(ords[i], glo * _QGROUP)] if sr else None)
                for moment, x, codes, scales in ((0, m, mq[i], ms[i]), (1, v.sqrt_(), sq[i], ss[i])):
                    gen = torch.Generator().manual_seed(
                        _mix64(group["seed"] ^ _mix64((ords[i] << 32 | step) * 2 + moment)) >> 1)
                    u = torch.rand(numel, generator=gen)[glo * _QGROUP:glo * _QGROUP + n]
                    c, sc = _quantize_e4m3_sr(x, u, nonneg=moment == 1)
                    codes.copy_(c)
                    scales.copy_(sc)

    @torch.no_grad()
    def decode_states(self, p):
        """``(exp_avg, exp_avg_sq)`` of parameter ``p`` as fp32 tensors of its shape and strides
        (copies): the dequantised 8-bit states, or the fp32 states themselves."""
        st = self.state[p]
        if "exp_avg_q" not in st:
            return st["exp_avg"].clone(memory_format=torch.preserve_format), \
                st["exp_avg_sq"].clone(memory_format=torch.preserve_format)
        out = []
        for name, square in (("exp_avg", False), ("exp_avg_sq", True)):
            x = _dequantize_e4m3(st[name + "_q"], st[name + "_scale"])
            t = _dense_like(p)
            _flat_range(t, 0, p.numel()).copy_(x * x if square else x)
            out.append(t)
        return tuple(out)

    def _cpu_step(self, ps, gs, m1, m2, masters, group, step, grad_scale, sr_keys=None):
        """``sr_keys``: per parameter (or range) its (ordinal, element offset within the parameter) where
        the write is stochastically rounded: the GPU's rounding and bits, given the same fp32 value."""
        b1, b2 = group["betas"]
        lr, eps, wd = group["lr"], group["eps"], group["weight_decay"]
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        for i, (p, g) in enumerate(zip(ps, gs)):
            w = masters[i] if masters else p.float()
            gg = g.float() * (grad_scale.float() if grad_scale is not None else 1.0)
            if group["maximize"]:
                gg = -gg
            if wd != 0:
                if self._decoupled:
                    w = w * (1 - lr * wd)
                else:
                    gg = gg + wd * w
            m1[i].mul_(b1).add_(gg, alpha=1 - b1)
            m2[i].mul_(b2).addcmul_(gg, gg, value=1 - b2)
            denom = (m2[i].sqrt() / (bc2 ** 0.5)).add_(eps)
            w = w - (lr / bc1) * m1[i] / denom
            if masters:
                masters[i].copy_(w)
            if sr_keys is not None:
                w = stochastic_round_bf16(w, group["seed"], sr_keys[i][0], step, sr_keys[i][1])
            p.copy_(w)


class FusedAdam(FusedAdamW):
    """Adam with L2 (coupled) weight decay."""

    _decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False,
                 master_weights=False, amsgrad=False, state_bits=32, seed=0, param_rounding="nearest"):
        super().__init__(params, lr, betas, eps, weight_decay, maximize, master_weights, amsgrad, state_bits, seed,
                         param_rounding)


def grad_norm(parameters: Iterable[torch.Tensor], max_norm: float = 0.0) -> torch.Tensor:
    """Total L2 norm of the grads (device scalar pair [norm, clip_coef]); no host sync on GPU."""
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor([0.0, 1.0])
    dev = grads[0].device
    if dev.type == "cuda":
        C = load()
        out = torch.empty(2, dtype=torch.float32, device=dev)
        by_dtype = defaultdict(list)
        for g in grads:
            by_dtype[g.dtype].append(g)
        if len(by_dtype) == 1:
            C.mt_l2norm(grads, out, float(max_norm))
            return out
        sq = torch.zeros(1, dtype=torch.float32, device=dev)
        for lst in by_dtype.values():
            C.mt_l2norm(lst, out, 0.0)
            sq += out[0] ** 2
        norm = sq.sqrt()
        coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0) if max_norm > 0 else torch.ones_like(norm)
        return torch.cat([norm, coef])
    norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g.float()) for g in grads]))
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0) if max_norm > 0 else torch.ones_like(norm)
    return torch.stack([norm, coef])


def clip_grad_norm_(parameters: Iterable[torch.Tensor], max_norm: float, fused_into_optimizer: bool = False):
    """Clip grads by total L2 norm (torch.nn.utils.clip_grad_norm_ semantics).

    Returns the total norm (device tensor). With ``fused_into_optimizer=True`` the grads are
    not touched; instead ``(norm, coef)`` is returned so ``optimizer.step(grad_scale=coef)``
    applies the clip inside the fused update (one pass less over the gradients).
    """
    params = [p for p in parameters if p.grad is not None]
    nc = grad_norm(params, max_norm)
    if fused_into_optimizer:
        return nc[0], nc[1:2]
    grads = [p.grad for p in params]
    if grads and grads[0].device.type == "cuda":
        C = load()
        by_dtype = defaultdict(list)
        for g in grads:
            by_dtype[g.dtype].append(g)
        for lst in by_dtype.values():
            C.mt_scale_copy(lst, lst, 1.0, nc[1:2].contiguous())
    else:
        for g in grads:
            g.mul_(nc[1].to(g.dtype))
    return nc[0]
