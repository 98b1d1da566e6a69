"""References shared by the stochastically-rounded-parameter tests (test_sr_params_cpu.py,
test_sr_params_gpu.py): the rounding's definition written out once more in numpy's wrapping unsigned
arithmetic (the package's CPU path emulates it in int64), crafted inputs, and bit views.

Definition under test (``stochastic_round_bf16(x, seed, ordinal, step, offset)``): for element i with
fp32 bits u and the 16 random bits r of element index e = offset + i, the result is the upper half of
u + r; a finite value whose sum would have an all-ones exponent keeps the upper half of u; +-inf stay,
NaN becomes the quiet NaN 0x7FC0. r = mix32(lo ^ kp ^ hi) >> 16 with lo = e mod 2^32,
hi = (e >> 32) * 0x9e3779b9 mod 2^32, key = mix64(seed ^ mix64(ordinal << 32 | step)) and
kp = mix64(key + 0x9e3779b97f4a7c15) mod 2^32.
"""
import numpy as np
import torch

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix64(z: int) -> int:  # splitmix64 finalizer
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix32(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def stream_keys(seed: int, ordinal: int, step: int):
    """(km, ks, kp): the two moment keys of the 8-bit states and the parameter write's key."""
    key = mix64(seed ^ mix64((ordinal << 32) | step))
    return key & 0xFFFFFFFF, key >> 32, mix64(key + GOLDEN) & 0xFFFFFFFF


def random16(n: int, seed: int, ordinal: int = 0, step: int = 0, offset: int = 0) -> np.ndarray:
    e = np.arange(offset, offset + n, dtype=np.uint64)
    lo = (e & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (e >> np.uint64(32)).astype(np.uint32) * np.uint32(0x9E3779B9)
    return mix32(lo ^ np.uint32(stream_keys(seed, ordinal, step)[2]) ^ hi) >> np.uint32(16)


def f32_bits(x: torch.Tensor) -> np.ndarray:
    return x.detach().cpu().contiguous().view(torch.int32).numpy().astype(np.uint32).ravel()


def bf16_bits(x: torch.Tensor) -> np.ndarray:
    return x.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.uint16).ravel()


def from_f32_bits(bits) -> torch.Tensor:
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.int32).copy()).view(torch.float32)


def ref_round_bits(x: torch.Tensor, seed: int, ordinal: int = 0, step: int = 0, offset: int = 0) -> np.ndarray:
    """bf16 bit patterns (uint16) of the definition applied to the contiguous fp32 ``x``."""
    u = f32_bits(x)
    with np.errstate(over="ignore"):
        t = u + random16(u.size, seed, ordinal, step, offset)
    full = np.uint32(0x7F800000)
    t = np.where((t & full) == full, u, t)  # (also +-inf: they keep their own bits)
    t = np.where(((u & full) == full) & ((u & np.uint32(0x007FFFFF)) != 0), np.uint32(0x7FC00000), t)
    return (t >> np.uint32(16)).astype(np.uint16)


def all_bf16_patterns() -> torch.Tensor:
    """Every bf16 bit pattern, widened to fp32 (65,536 values: NaNs and infinities included)."""
    return from_f32_bits(np.arange(1 << 16, dtype=np.uint32) << np.uint32(16))


def crafted() -> torch.Tensor:
    """Every bf16 pattern, the largest finite fp32 of both signs, values one fp32 step from a bf16,
    NaNs with payload in the low half only, the smallest subnormals, and both zeros."""
    extra = [0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0001, 0xFF7F8000, 0x3F800001, 0x3F80FFFF, 0xBF808000, 0x7F800001,
             0xFF80FFFF, 0x7FFFFFFF, 0xFFFFFFFF, 0x00000001, 0x80000001, 0x0000FFFF, 0x00000000, 0x80000000]
    return torch.cat([all_bf16_patterns(), from_f32_bits(extra)])


def random_f32(n: int, seed: int) -> torch.Tensor:
    """Finite fp32 values over many binades, both signs."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=gen) * torch.exp2(torch.randint(-20, 21, (n,), generator=gen).float())
