// Per-tensor FP8 casts for the opt-in FP8 linear layers (ops/fp8.py, gemm_fp8.hip):
//
//   fp8_amax(x)                         max |x| of a bf16 tensor -> float32[1]
//   fp8_quantize(x[R, C], amax, fmt, T) q[R, C] (and qT[C, R]) = fp8(clamp(x · scale, ±FMAX)),
//                                       scale = FMAX / amax (1 for an all-zero tensor)
//
// OCP encodings (gfx950): fmt 0 = e4m3 (FMAX 448), 1 = e5m2 (FMAX 57344), round-to-nearest-even via
// v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32, after an explicit clamp (the conversion's overflow mode is
// never relied on). amax and scale stay on the device and nothing syncs the host, so the casts are
// capturable into a HIP graph. The transposed copy comes from the same pass: a 64 x 64 tile of
// bytes goes through LDS, global reads and both global writes are 16 B per lane.
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include "common.h"
#include "kernels/dev_utils.h"
#include "kernels/norm.h"

namespace xddp {
namespace kernels {

namespace {

using dev::u32x4;

constexpr int kAmaxThreads = 256;

// |x| of non-negative floats orders like their bit patterns: the block's maximum goes out with one
// vector atomicMax on the uint bits (bf16 -> f32 is exact, so the result is max |x| exactly).
__global__ __launch_bounds__(kAmaxThreads) void fp8_amax_kernel(const uint16_t* __restrict__ x, int64_t n,
                                                                unsigned* __restrict__ out) {
  __shared__ float red[kAmaxThreads / 64];
  const int64_t stride = (int64_t)gridDim.x * kAmaxThreads, n8 = n / 8;
  uint32_t m = 0;  // max of the 15-bit magnitudes, in either half of a packed pair
  for (int64_t i = (int64_t)blockIdx.x * kAmaxThreads + threadIdx.x; i < n8; i += stride) {
    const u32x4 v = reinterpret_cast<const u32x4*>(x)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) m = max(m, max(v[e] & 0x7fffu, (v[e] >> 16) & 0x7fffu));
  }
  for (int64_t i = n8 * 8 + (int64_t)blockIdx.x * kAmaxThreads + threadIdx.x; i < n; i += stride)
    m = max(m, (uint32_t)(x[i] & 0x7fffu));
  float f = dev::wave_max(__uint_as_float(m << 16));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = f;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kAmaxThreads / 64; ++w) f = fmaxf(f, red[w]);
    atomicMax(out, __float_as_uint(f));
  }
}

constexpr int kQT = 64, kQThreads = 256, kQStride = kQT + 4;  // LDS tile rows padded by one dword

template <int FMT>
__device__ __forceinline__ uint32_t cvt4(float a, float b, float c, float d) {
  int r = 0;
  if (FMT == 0) {
    r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, r, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
  } else {
    r = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, r, false);
    r = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, r, true);
  }
  return (uint32_t)r;
}

// One 64 x 64 tile per block; thread t converts 16 consecutive elements of tile row t / 4 (two 16-B
// reads, one 16-B write of q) and, with TR, writes 16 consecutive bytes of tile column t / 4 to qT.
// R and C are multiples of 16, so a 16-element chunk is either whole or absent at the edges.
template <int FMT, bool TR>
__global__ __launch_bounds__(kQThreads) void fp8_quantize_kernel(const uint16_t* __restrict__ x,
                                                                 const float* __restrict__ amax,
                                                                 uint8_t* __restrict__ q, uint8_t* __restrict__ qT,
                                                                 float* __restrict__ scale_out, int64_t R, int64_t C) {
  constexpr float FMAX = FMT == 0 ? 448.f : 57344.f;
  __shared__ __attribute__((aligned(16))) uint8_t tile[TR ? kQT * kQStride : 16];
  const float am = amax[0];
  // (the lower bound keeps the quotient finite for denormal-sized maxima)
  const float scale = am > 0.f ? FMAX / fmaxf(am, 1e-30f) : 1.f;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) scale_out[0] = scale;
  const int64_t r0 = (int64_t)blockIdx.y * kQT, c0 = (int64_t)blockIdx.x * kQT;
  const int tr = threadIdx.x >> 2, tc = threadIdx.x & 3;
  const int64_t row = r0 + tr, col = c0 + tc * 16;
  if (row < R && col < C) {
    const u32x4* src = reinterpret_cast<const u32x4*>(x + row * C + col);
    const u32x4 lo = src[0], hi = src[1];
    float f[16];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      f[2 * e] = __uint_as_float(lo[e] << 16);
      f[2 * e + 1] = __uint_as_float(lo[e] & 0xffff0000u);
      f[8 + 2 * e] = __uint_as_float(hi[e] << 16);
      f[8 + 2 * e + 1] = __uint_as_float(hi[e] & 0xffff0000u);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) f[e] = fminf(fmaxf(f[e] * scale, -FMAX), FMAX);
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = cvt4<FMT>(f[4 * e], f[4 * e + 1], f[4 * e + 2], f[4 * e + 3]);
    *reinterpret_cast<u32x4*>(q + row * C + col) = o;
    if (TR) {
      uint32_t* t = reinterpret_cast<uint32_t*>(tile + tr * kQStride + tc * 16);
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = o[e];
    }
  }
  if (TR) {
    __syncthreads();
    // tile column tr, tile rows tc * 16 .. + 15 -> qT[c0 + tr][r0 + tc * 16 ..]
    const int64_t trow = c0 + tr, tcol = r0 + tc * 16;
    if (trow < C && tcol < R) {
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        uint32_t w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) w |= (uint32_t)tile[(tc * 16 + 4 * e + b) * kQStride + tr] << (8 * b);
        o[e] = w;
      }
      *reinterpret_cast<u32x4*>(qT + trow * R + tcol) = o;
    }
  }
}

}  // namespace

at::Tensor fp8_amax(const at::Tensor& x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous() &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "fp8_amax: a contiguous, 16-B aligned bf16 CUDA tensor expected");
  auto out = at::empty({1}, x.options().dtype(at::kFloat));
  auto stream = c10::hip::getCurrentHIPStream(x.device().index()).stream();
  XDDP_HIP_CHECK(hipMemsetAsync(out.data_ptr(), 0, sizeof(float), stream));
  const int64_t n = x.numel();
  if (n == 0) return out;
  const int blocks = (int)std::min<int64_t>((n / 8 + kAmaxThreads - 1) / kAmaxThreads + 1, 2048);
  hipLaunchKernelGGL(fp8_amax_kernel, dim3(blocks), dim3(kAmaxThreads), 0, stream,
                     reinterpret_cast<const uint16_t*>(x.data_ptr()), n, reinterpret_cast<unsigned*>(out.data_ptr()));
  XDDP_HIP_CHECK(hipGetLastError());
  return out;
}

std::tuple<at::Tensor, c10::optional<at::Tensor>, at::Tensor> fp8_quantize(const at::Tensor& x, const at::Tensor& amax,
                                                                           int64_t fmt, bool transpose) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2 && x.is_contiguous() &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "fp8_quantize: a contiguous, 16-B aligned bf16 CUDA matrix expected");
  const int64_t R = x.size(0), C = x.size(1);
  TORCH_CHECK(R > 0 && C > 0 && R % 16 == 0 && C % 16 == 0,
              "fp8_quantize: rows and columns must be positive multiples of 16, got [", R, ", ", C, "]");
  TORCH_CHECK(amax.is_cuda() && amax.scalar_type() == at::kFloat && amax.numel() == 1,
              "fp8_quantize: amax must be a float32[1] CUDA tensor");
  TORCH_CHECK(fmt == 0 || fmt == 1, "fp8_quantize: fmt is 0 (e4m3) or 1 (e5m2)");
  const int64_t gx = (C + kQT - 1) / kQT, gy = (R + kQT - 1) / kQT;
  const auto bopts = x.options().dtype(at::kByte);
  at::Tensor q = at::empty({R, C}, bopts), qT = transpose ? at::empty({C, R}, bopts) : at::Tensor();
  at::Tensor scale = at::empty({1}, x.options().dtype(at::kFloat));
  auto stream = c10::hip::getCurrentHIPStream(x.device().index()).stream();
  TORCH_CHECK(gy <= 65535, "fp8_quantize: more than 65535 x 64 rows are not supported");
  const dim3 grid((unsigned)gx, (unsigned)gy);
  const auto* xp = reinterpret_cast<const uint16_t*>(x.data_ptr());
  auto* qp = reinterpret_cast<uint8_t*>(q.data_ptr());
  auto* tp = transpose ? reinterpret_cast<uint8_t*>(qT.data_ptr()) : nullptr;
#define XDDP_Q(FMT_, TR_)                                                                                        \
  hipLaunchKernelGGL((fp8_quantize_kernel<FMT_, TR_>), grid, dim3(kQThreads), 0, stream, xp, amax.data_ptr<float>(), \
                     qp, tp, scale.data_ptr<float>(), R, C)
  if (fmt == 0) {
    if (transpose) XDDP_Q(0, true); else XDDP_Q(0, false);
  } else {
    if (transpose) XDDP_Q(1, true); else XDDP_Q(1, false);
  }
#undef XDDP_Q
  XDDP_HIP_CHECK(hipGetLastError());
  return {q, transpose ? c10::optional<at::Tensor>(qT) : c10::nullopt, scale};
}

}  // namespace kernels
}  // namespace xddp
