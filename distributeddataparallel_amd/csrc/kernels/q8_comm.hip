// 8-bit block-quantized gradient wire: quantize, dequantize-and-average, reduce-and-requantize.
//
// Format. A bucket of n elements is cut into blocks of G consecutive elements (G = 128 | 256 |
// 512 | 1024, the last block may be short). For a block of finite values whose hi - lo is finite
// (lo = min, hi = max over the block's real elements):
//
//   scale = (hi - lo) / 255                          (fp32 division)
//   code  = clamp(rint((x - lo) / scale), 0, 255)    (0 everywhere when scale == 0)
//   x'    = fmaf(code, scale, lo)
//
// A block that holds a NaN or an inf, or whose hi - lo overflows, stores scale = NaN: all of it
// decodes to NaN on every rank and an overflow check downstream still sees it. Elements past n
// take no part in min / max and get code 0.
//
// Payload: S segments of cb blocks; a segment is cb·G code bytes, then cb (lo, scale) fp32 pairs,
// so one collective moves codes and parameters together and the pairs stay 8-byte aligned.
//
// Work split, shared by the three kernels: one wave owns one block, lane l holds the G / 64
// consecutive elements [l·G/64, (l + 1)·G/64) in registers (G = 512: 8 elements, one 16-byte load
// of bf16 / fp16, two of fp32, one 8-byte store of codes). Min, max and the averaged values never
// leave registers; min / max fold over the wave with __shfl_xor, the non-finite flag with one
// ballot: no LDS, no barrier. A 256-thread workgroup carries 4 independent blocks and the grid is
// sized to the CU count and strides over the blocks. The block index is wave-uniform, so a
// segment's (lo, scale) pair is one uniform 8-byte load. 16-byte accesses to the bucket are used
// only when its base is 16-byte aligned and the block is whole; otherwise the same kernel goes
// element by element with a bound check (a view at an odd offset, the tail block).
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <algorithm>
#include <cfloat>

#include "common.h"
#include "kernels/dev_utils.h"
#include "kernels/lane_vec.h"
#include "kernels/q8_comm.h"

namespace xddp {
namespace kernels {

namespace {

constexpr int kQT = 256;           // threads per workgroup
constexpr int kQW = kQT / 64;      // waves = blocks of the format per workgroup round
constexpr int kQGroupsPerCU = 8;   // 32 waves per CU: the kernels hold few registers

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

using dev::LaneVec;  // a lane's E elements of the bucket as fp32 (kernels/lane_vec.h)

// a lane's E code bytes, packed 4 to a word (p is aligned to min(8, E) bytes: segments start at
// multiples of 8 bytes, not of 16)
template <int E>
struct LaneCodes {
  static constexpr int NW = (E + 3) / 4;
  static __device__ __forceinline__ void ld(const uint8_t* p, uint32_t (&w)[NW]) {
    if constexpr (E == 2) {
      w[0] = *reinterpret_cast<const uint16_t*>(p);
    } else if constexpr (E == 4) {
      w[0] = *reinterpret_cast<const uint32_t*>(p);
    } else {
#pragma unroll
      for (int j = 0; j < E / 8; ++j) {
        const uint2 t = reinterpret_cast<const uint2*>(p)[j];
        w[2 * j] = t.x;
        w[2 * j + 1] = t.y;
      }
    }
  }
  static __device__ __forceinline__ void st(uint8_t* p, const uint32_t (&w)[NW]) {
    if constexpr (E == 2) {
      *reinterpret_cast<uint16_t*>(p) = (uint16_t)w[0];
    } else if constexpr (E == 4) {
      *reinterpret_cast<uint32_t*>(p) = w[0];
    } else {
#pragma unroll
      for (int j = 0; j < E / 8; ++j) reinterpret_cast<uint2*>(p)[j] = make_uint2(w[2 * j], w[2 * j + 1]);
    }
  }
};

// One segment's view of block b: the lane's codes and the block's (lo, scale) pair.
template <int G>
struct Slot {
  uint8_t* codes;
  float2* param;
  __device__ __forceinline__ Slot(uint8_t* seg, unsigned cb, unsigned b, int lane)
      : codes(seg + (int64_t)b * G + lane * (G / 64)),
        param(reinterpret_cast<float2*>(seg + (int64_t)cb * G) + b) {}
};

// Quantize the block whose elements the wave holds in v (bit k of `valid`: element k is real;
// the others are 0) and store codes and parameters. Every lane of the wave calls this.
template <int G>
__device__ __forceinline__ void quantize_block(const float (&v)[G / 64], unsigned valid, const Slot<G>& s, int lane) {
  constexpr int E = G / 64;
  float lo = INFINITY, hi = -INFINITY;
  bool nonfinite = false;
#pragma unroll
  for (int k = 0; k < E; ++k)
    if (valid >> k & 1u) {
      lo = fminf(lo, v[k]);  // fminf / fmaxf drop a NaN: the flag keeps it
      hi = fmaxf(hi, v[k]);
      nonfinite |= !(fabsf(v[k]) <= FLT_MAX);
    }
  lo = wave_min(lo);
  hi = dev::wave_max(hi);
  const float range = hi - lo;
  const bool bad = __ballot(nonfinite) != 0ull || !(range <= FLT_MAX);
  const float scale = bad ? __uint_as_float(0x7fc00000u) : range / 255.f;
  uint32_t w[LaneCodes<E>::NW];
#pragma unroll
  for (int j = 0; j < LaneCodes<E>::NW; ++j) w[j] = 0u;
  if (scale > 0.f) {  // not for a constant block (scale 0) or a NaN scale: their codes are 0
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const float c = fminf(fmaxf(rintf((v[k] - lo) / scale), 0.f), 255.f);
      w[k / 4] |= (valid >> k & 1u ? (uint32_t)c : 0u) << (8 * (k % 4));
    }
  }
  LaneCodes<E>::st(s.codes, w);
  if (lane == 0) *s.param = make_float2(lo, scale);
}

// acc = mean over W segments (each `stride` bytes after the one before) of the decoded block b:
// fmaf(code, scale, lo) accumulated in segment order, then one division, on every rank alike.
template <int G>
__device__ __forceinline__ void decode_mean(const uint8_t* seg, int64_t stride, unsigned cb, unsigned b, int W,
                                            int lane, float (&acc)[G / 64]) {
  constexpr int E = G / 64;
#pragma unroll
  for (int k = 0; k < E; ++k) acc[k] = 0.f;
  for (int r = 0; r < W; ++r, seg += stride) {
    const Slot<G> s(const_cast<uint8_t*>(seg), cb, b, lane);
    const float2 p = *s.param;
    uint32_t w[LaneCodes<E>::NW];
    LaneCodes<E>::ld(s.codes, w);
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] += fmaf((float)(w[k / 4] >> (8 * (k % 4)) & 0xffu), p.y, p.x);
  }
  if (W > 1) {
    const float fw = (float)W;
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] = acc[k] / fw;
  }
}

// wave-uniform index of this wave among all waves of the grid
__device__ __forceinline__ unsigned first_block() {
  return blockIdx.x * kQW + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// x [n] -> payload of total = S·cb blocks, of which the first nb are real
template <typename T, int G>
__global__ __launch_bounds__(kQT) void q8_quantize_kernel(const T* __restrict__ x, uint8_t* __restrict__ payload,
                                                          int64_t n, unsigned nb, unsigned cb, unsigned total,
                                                          int vec) {
  constexpr int E = G / 64;
  const int lane = threadIdx.x & 63;
  for (unsigned gb = first_block(); gb < total; gb += gridDim.x * kQW) {
    const unsigned seg = gb / cb, b = gb - seg * cb;
    const Slot<G> s(payload + (int64_t)seg * cb * (G + 8), cb, b, lane);
    if (gb >= nb) {  // padding block: codes 0, parameters (0, 0)
      uint32_t w[LaneCodes<E>::NW];
#pragma unroll
      for (int j = 0; j < LaneCodes<E>::NW; ++j) w[j] = 0u;
      LaneCodes<E>::st(s.codes, w);
      if (lane == 0) *s.param = make_float2(0.f, 0.f);
      continue;
    }
    const int64_t e0 = (int64_t)gb * G + lane * E;
    float v[E];
    unsigned valid = (1u << E) - 1u;
    if (vec && ((int64_t)gb + 1) * G <= n) {
      LaneVec<T, E>::ld(x + e0, v);
    } else {
      valid = 0u;
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const bool in = e0 + k < n;
        v[k] = in ? dev::Elem<T, float>::ld(x, e0 + k) : 0.f;
        valid |= in ? 1u << k : 0u;
      }
    }
    quantize_block<G>(v, valid, s, lane);
  }
}

// mean (W segments over the same nb blocks) or concat (W = 1, block gb lives in segment gb / cb)
template <typename T, int G>
__global__ __launch_bounds__(kQT) void q8_dequant_kernel(const uint8_t* __restrict__ payload, T* __restrict__ out,
                                                         int64_t n, unsigned nb, unsigned cb, int W, int concat,
                                                         int vec) {
  constexpr int E = G / 64;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)cb * (G + 8);
  for (unsigned gb = first_block(); gb < nb; gb += gridDim.x * kQW) {
    const unsigned seg = concat ? gb / cb : 0u, b = gb - seg * cb;
    float acc[E];
    decode_mean<G>(payload + seg * stride, stride, cb, b, W, lane, acc);
    const int64_t e0 = (int64_t)gb * G + lane * E;
    if (vec && ((int64_t)gb + 1) * G <= n) {
      LaneVec<T, E>::st(out + e0, acc);
    } else {
#pragma unroll
      for (int k = 0; k < E; ++k)
        if (e0 + k < n) dev::Elem<T, float>::st(out, e0 + k, acc[k]);
    }
  }
}

// W segments of cb blocks -> one segment: the mean stays in registers and is quantized again
template <int G>
__global__ __launch_bounds__(kQT) void q8_reduce_requant_kernel(const uint8_t* __restrict__ in,
                                                                uint8_t* __restrict__ out, unsigned cb, int W) {
  constexpr int E = G / 64;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)cb * (G + 8);
  for (unsigned b = first_block(); b < cb; b += gridDim.x * kQW) {
    float acc[E];
    decode_mean<G>(in, stride, cb, b, W, lane, acc);
    quantize_block<G>(acc, (1u << E) - 1u, Slot<G>(out, cb, b, lane), lane);
  }
}

// ---- host --------------------------------------------------------------------------------------
int cu_count(int device) {
  int v = 0;
  return hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && v > 0 ? v : 256;
}

dim3 grid_for(int64_t blocks, int device) {
  const int64_t groups = (blocks + kQW - 1) / kQW;
  return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(groups, (int64_t)cu_count(device) * kQGroupsPerCU)));
}

void check_block(const char* op, int64_t block, int64_t segments) {
  TORCH_CHECK(block == 128 || block == 256 || block == 512 || block == 1024, op,
              ": block must be 128, 256, 512 or 1024, got ", block);
  TORCH_CHECK(segments >= 1 && segments <= 65536, op, ": segments must be in [1, 65536], got ", segments);
}

void check_payload(const char* op, const char* name, const at::Tensor& p, const at::Device& device) {
  TORCH_CHECK(p.is_cuda() && p.device() == device && p.scalar_type() == at::kByte && p.dim() == 1 &&
                  p.is_contiguous(),
              op, ": ", name, " must be a flat contiguous uint8 tensor on ", device);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(p.data_ptr()) % 8 == 0, op, ": ", name, " must be 8-byte aligned");
}

void check_bucket(const char* op, const char* name, const at::Tensor& t) {
  const auto st = t.scalar_type();
  TORCH_CHECK(t.is_cuda() && t.dim() == 1 && t.is_contiguous() &&
                  (st == at::kFloat || st == at::kBFloat16 || st == at::kHalf),
              op, ": ", name, " must be a flat contiguous fp32 / bf16 / fp16 CUDA tensor");
  TORCH_CHECK(t.numel() < (int64_t(1) << 37), op, ": ", name, " has too many elements");  // blocks fit 32 bits
}

bool aligned16(const at::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }

#define XDDP_Q8_BLOCK_SWITCH(block, ...)    \
  switch (block) {                          \
    case 128: { constexpr int G = 128; __VA_ARGS__; break; }   \
    case 256: { constexpr int G = 256; __VA_ARGS__; break; }   \
    case 512: { constexpr int G = 512; __VA_ARGS__; break; }   \
    default: { constexpr int G = 1024; __VA_ARGS__; break; }   \
  }

template <typename T>
void launch_quantize(const at::Tensor& x, at::Tensor& payload, int64_t block, unsigned nb, unsigned cb, unsigned total,
                     hipStream_t stream) {
  const dim3 grid = grid_for(total, x.device().index());
  XDDP_Q8_BLOCK_SWITCH(block, hipLaunchKernelGGL((q8_quantize_kernel<T, G>), grid, dim3(kQT), 0, stream,
                                                 reinterpret_cast<const T*>(x.data_ptr()),
                                                 payload.data_ptr<uint8_t>(), x.numel(), nb, cb, total,
                                                 aligned16(x) ? 1 : 0));
}

template <typename T>
void launch_dequant(const at::Tensor& payload, at::Tensor& out, int64_t block, unsigned nb, unsigned cb, int W,
                    int concat, hipStream_t stream) {
  const dim3 grid = grid_for(nb, out.device().index());
  XDDP_Q8_BLOCK_SWITCH(block, hipLaunchKernelGGL((q8_dequant_kernel<T, G>), grid, dim3(kQT), 0, stream,
                                                 payload.data_ptr<uint8_t>(), reinterpret_cast<T*>(out.data_ptr()),
                                                 out.numel(), nb, cb, W, concat, aligned16(out) ? 1 : 0));
}

}  // namespace

void q8_quantize(const at::Tensor& x, at::Tensor payload, int64_t block, int64_t segments) {
  check_block("q8_quantize", block, segments);
  check_bucket("q8_quantize", "x", x);
  check_payload("q8_quantize", "payload", payload, x.device());
  const int64_t n = x.numel(), nb = (n + block - 1) / block, cb = (nb + segments - 1) / segments;
  TORCH_CHECK(payload.numel() == segments * cb * (block + 8), "q8_quantize: payload must hold ",
              segments * cb * (block + 8), " bytes (", segments, " segments of ", cb, " blocks), got ",
              payload.numel());
  TORCH_CHECK(segments * cb < (int64_t(1) << 31), "q8_quantize: too many blocks");
  if (n == 0) return;
  auto stream = c10::hip::getCurrentHIPStream(x.device().index()).stream();
  const unsigned unb = (unsigned)nb, ucb = (unsigned)cb, total = (unsigned)(segments * cb);
  if (x.scalar_type() == at::kFloat) launch_quantize<float>(x, payload, block, unb, ucb, total, stream);
  else if (x.scalar_type() == at::kBFloat16) launch_quantize<dev::bf16_t>(x, payload, block, unb, ucb, total, stream);
  else launch_quantize<dev::f16_t>(x, payload, block, unb, ucb, total, stream);
  XDDP_HIP_CHECK(hipGetLastError());
}

void q8_dequantize_mean(const at::Tensor& payload, at::Tensor out, int64_t block, int64_t segments,
                        const std::string& mode) {
  check_block("q8_dequantize_mean", block, segments);
  TORCH_CHECK(mode == "mean" || mode == "concat", "q8_dequantize_mean: mode must be \"mean\" or \"concat\", got \"",
              mode, "\"");
  check_bucket("q8_dequantize_mean", "out", out);
  check_payload("q8_dequantize_mean", "payload", payload, out.device());
  const bool concat = mode == "concat";
  const int64_t n = out.numel(), nb = (n + block - 1) / block;
  const int64_t cb = concat ? (nb + segments - 1) / segments : nb;
  TORCH_CHECK(payload.numel() == segments * cb * (block + 8), "q8_dequantize_mean: payload must hold ",
              segments * cb * (block + 8), " bytes (", segments, " segments of ", cb, " blocks), got ",
              payload.numel());
  TORCH_CHECK(segments * cb < (int64_t(1) << 31), "q8_dequantize_mean: too many blocks");
  if (n == 0) return;
  auto stream = c10::hip::getCurrentHIPStream(out.device().index()).stream();
  const int W = concat ? 1 : (int)segments;
  const unsigned unb = (unsigned)nb, ucb = (unsigned)cb;
  if (out.scalar_type() == at::kFloat) launch_dequant<float>(payload, out, block, unb, ucb, W, concat, stream);
  else if (out.scalar_type() == at::kBFloat16)
    launch_dequant<dev::bf16_t>(payload, out, block, unb, ucb, W, concat, stream);
  else launch_dequant<dev::f16_t>(payload, out, block, unb, ucb, W, concat, stream);
  XDDP_HIP_CHECK(hipGetLastError());
}

void q8_reduce_requant(const at::Tensor& payload_in, at::Tensor payload_out, int64_t block, int64_t segments) {
  check_block("q8_reduce_requant", block, segments);
  TORCH_CHECK(payload_in.is_cuda(), "q8_reduce_requant: payload_in must be a CUDA tensor");
  check_payload("q8_reduce_requant", "payload_in", payload_in, payload_in.device());
  check_payload("q8_reduce_requant", "payload_out", payload_out, payload_in.device());
  const int64_t seg = payload_out.numel();
  TORCH_CHECK(seg % (block + 8) == 0 && payload_in.numel() == segments * seg,
              "q8_reduce_requant: payload_out must hold whole blocks of ", block + 8, " bytes and payload_in ",
              segments, " such segments, got ", seg, " and ", payload_in.numel(), " bytes");
  const int64_t cb = seg / (block + 8);
  TORCH_CHECK(cb < (int64_t(1) << 31), "q8_reduce_requant: too many blocks");
  if (cb == 0) return;
  auto stream = c10::hip::getCurrentHIPStream(payload_in.device().index()).stream();
  const dim3 grid = grid_for(cb, payload_in.device().index());
  XDDP_Q8_BLOCK_SWITCH(block, hipLaunchKernelGGL((q8_reduce_requant_kernel<G>), grid, dim3(kQT), 0, stream,
                                                 payload_in.data_ptr<uint8_t>(), payload_out.data_ptr<uint8_t>(),
                                                 (unsigned)cb, (int)segments));
  XDDP_HIP_CHECK(hipGetLastError());
}

}  // namespace kernels
}  // namespace xddp
