// 1-bit gradient wire with error feedback: compress, decode-and-average, reduce-and-recompress.
//
// Format. A bucket of n elements is cut into blocks of G consecutive elements (G = 512 | 1024 |
// 2048, the last block may be short). For a block with c >= 1 real elements x_i and an fp32
// residual e_i:
//
//   v_i   = float(x_i) + e_i
//   scale = (sum_i |v_i|) / c            (fp32; the l2-optimal scale for sign(v))
//   bit_i = v_i < 0                      (+0, -0 and padding give bit 0)
//   d_i   = bit_i ? -scale : +scale      (the decoded value)
//   e_i  <- v_i - d_i
//
// Element i of a block is bit i % 8 of byte i / 8. A block whose v holds a NaN or an inf, or whose
// |v| sum overflows, stores scale = NaN and zero bits and leaves its e_i as they were: it decodes to
// NaN on every rank, and one skipped step does not poison the residual. An all-zero block has
// scale 0 and decodes to exact zeros.
//
// Payload: S segments of cb blocks; a segment is cb·G/8 sign bytes, then cb fp32 scales. Padding
// blocks hold zero bytes and scale 0.
//
// Work split, shared by the three kernels: one wave owns one block, lane l holds the E = G / 64
// consecutive elements [l·E, (l + 1)·E) in registers, so its sign bits are E / 8 whole bytes (one
// 1-, 2- or 4-byte store) and a wave writes G / 8 contiguous bytes. |v| is summed over the lane's
// elements in order and then over the wave by a __shfl_xor butterfly, which leaves the same bits in
// every lane: a block's bytes depend on nothing but the block. No LDS, no barrier, no atomics. A
// 256-thread workgroup carries 4 independent blocks and the grid is sized to the CU count and
// strides over the blocks. The block index is wave-uniform, so a block's scale is one uniform load.
// 16-byte accesses to the bucket and the residual are used only when both bases are 16-byte aligned
// and the block is whole; otherwise the same kernel goes element by element with a bound check.
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <algorithm>
#include <cfloat>

#include "common.h"
#include "kernels/dev_utils.h"
#include "kernels/lane_vec.h"
#include "kernels/onebit_comm.h"

namespace xddp {
namespace kernels {

namespace {

constexpr int kOT = 256;           // threads per workgroup
constexpr int kOW = kOT / 64;      // waves = blocks of the format per workgroup round
constexpr int kOGroupsPerCU = 8;   // 32 waves per CU

using dev::LaneVec;

// a lane's E sign bits: E / 8 bytes at p (aligned to E / 8 bytes), bit k in bit k of the word
template <int E>
__device__ __forceinline__ uint32_t ld_bits(const uint8_t* p) {
  if constexpr (E == 8) return *p;
  else if constexpr (E == 16) return *reinterpret_cast<const uint16_t*>(p);
  else return *reinterpret_cast<const uint32_t*>(p);
}
template <int E>
__device__ __forceinline__ void st_bits(uint8_t* p, uint32_t w) {
  if constexpr (E == 8) *p = (uint8_t)w;
  else if constexpr (E == 16) *reinterpret_cast<uint16_t*>(p) = (uint16_t)w;
  else *reinterpret_cast<uint32_t*>(p) = w;
}

template <int G>
constexpr int64_t block_bytes() { return G / 8 + 4; }

// One segment's view of block b: the lane's sign bytes and the block's scale.
template <int G>
struct Slot {
  uint8_t* bits;
  float* scale;
  __device__ __forceinline__ Slot(uint8_t* seg, unsigned cb, unsigned b, int lane)
      : bits(seg + (int64_t)b * (G / 8) + lane * (G / 512)),
        scale(reinterpret_cast<float*>(seg + (int64_t)cb * (G / 8)) + b) {}
  __device__ __forceinline__ void zero(int lane) const {  // a padding block
    st_bits<G / 64>(bits, 0u);
    if (lane == 0) *scale = 0.f;
  }
};

// +scale or -scale: the sign bit goes into the scale's sign by XOR
__device__ __forceinline__ float signed_scale(uint32_t scale_bits, uint32_t w, int k) {
  return __uint_as_float(scale_bits ^ ((w >> k & 1u) << 31));
}

// Compress the block whose v = x + e the wave holds (bit k of `valid`: element k is real; the
// others are 0; c real elements in the block), store bits and scale, and write e <- v - d to
// err[0 .. E) (`vec`: all E at once). Every lane of the wave calls this.
template <int G>
__device__ __forceinline__ void compress_block(const float (&v)[G / 64], uint32_t valid, int c, float* err, bool vec,
                                               const Slot<G>& s, int lane) {
  constexpr int E = G / 64;
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < E; ++k) sum += fabsf(v[k]);  // padding adds +0
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  // |v| has no cancellation: the sum is finite exactly when every v is and nothing overflowed
  const bool bad = !(sum <= FLT_MAX);
  const float scale = bad ? __uint_as_float(0x7fc00000u) : sum / (float)c;
  uint32_t w = 0u;
  if (!bad) {
#pragma unroll
    for (int k = 0; k < E; ++k) w |= (v[k] < 0.f ? 1u : 0u) << k;
  }
  st_bits<E>(s.bits, w);
  if (lane == 0) *s.scale = scale;
  if (bad) return;  // the residual of a skipped block stays as it was
  const uint32_t sb = __float_as_uint(scale);
  if (vec) {
    uint32_t e[E];
#pragma unroll
    for (int k = 0; k < E; ++k) e[k] = __float_as_uint(v[k] - signed_scale(sb, w, k));
    dev::st_words<E>(err, e);
  } else {
#pragma unroll
    for (int k = 0; k < E; ++k)
      if (valid >> k & 1u) err[k] = v[k] - signed_scale(sb, w, k);
  }
}

// acc = mean over W segments (each `stride` bytes after the one before) of the decoded block b:
// ((d_0 + d_1) + ...) + d_{W-1} in segment order, then one division, on every rank alike.
template <int G>
__device__ __forceinline__ void decode_mean(const uint8_t* seg, int64_t stride, unsigned cb, unsigned b, int W,
                                            int lane, float (&acc)[G / 64]) {
  constexpr int E = G / 64;
  for (int r = 0; r < W; ++r, seg += stride) {
    const Slot<G> s(const_cast<uint8_t*>(seg), cb, b, lane);
    const uint32_t sb = __float_as_uint(*s.scale);
    const uint32_t w = ld_bits<E>(s.bits);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const float d = signed_scale(sb, w, k);
      acc[k] = r == 0 ? d : acc[k] + d;
    }
  }
  if (W > 1) {
    const float fw = (float)W;
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] = acc[k] / fw;
  }
}

// wave-uniform index of this wave among all waves of the grid
__device__ __forceinline__ unsigned first_block() {
  return blockIdx.x * kOW + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// x [n], err [n] -> payload of total = S·cb blocks, of which the first nb are real
template <typename T, int G>
__global__ __launch_bounds__(kOT) void onebit_compress_kernel(const T* __restrict__ x, float* __restrict__ err,
                                                              uint8_t* __restrict__ payload, int64_t n, unsigned nb,
                                                              unsigned cb, unsigned total, int vec) {
  constexpr int E = G / 64;
  const int lane = threadIdx.x & 63;
  for (unsigned gb = first_block(); gb < total; gb += gridDim.x * kOW) {
    const unsigned seg = gb / cb, b = gb - seg * cb;
    const Slot<G> s(payload + (int64_t)seg * cb * block_bytes<G>(), cb, b, lane);
    if (gb >= nb) {
      s.zero(lane);
      continue;
    }
    const int64_t left = n - (int64_t)gb * G;  // >= 1
    const int64_t e0 = (int64_t)gb * G + lane * E;
    const bool whole = vec && left >= G;
    float v[E];
    uint32_t valid = 0xffffffffu >> (32 - E);
    if (whole) {
      float e[E];
      LaneVec<T, E>::ld(x + e0, v);
      LaneVec<float, E>::ld(err + e0, e);
#pragma unroll
      for (int k = 0; k < E; ++k) v[k] += e[k];
    } else {
      valid = 0u;
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const bool in = e0 + k < n;
        v[k] = in ? dev::Elem<T, float>::ld(x, e0 + k) + err[e0 + k] : 0.f;
        valid |= in ? 1u << k : 0u;
      }
    }
    compress_block<G>(v, valid, left < G ? (int)left : G, err + e0, whole, s, lane);
  }
}

// mean (W segments over the same nb blocks) or concat (W = 1, block gb lives in segment gb / cb)
template <typename T, int G>
__global__ __launch_bounds__(kOT) void onebit_decode_kernel(const uint8_t* __restrict__ payload, T* __restrict__ out,
                                                            int64_t n, unsigned nb, unsigned cb, int W, int concat,
                                                            int vec) {
  constexpr int E = G / 64;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)cb * block_bytes<G>();
  for (unsigned gb = first_block(); gb < nb; gb += gridDim.x * kOW) {
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

// W segments of cb blocks -> one segment: the mean stays in registers, takes the server residual
// err [cb·G] and is compressed again; the chunk's elements from `numel` on are padding
template <int G>
__global__ __launch_bounds__(kOT) void onebit_reduce_recompress_kernel(const uint8_t* __restrict__ in,
                                                                       float* __restrict__ err,
                                                                       uint8_t* __restrict__ out, unsigned cb, int W,
                                                                       int64_t numel, int vec) {
  constexpr int E = G / 64;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)cb * block_bytes<G>();
  for (unsigned b = first_block(); b < cb; b += gridDim.x * kOW) {
    const Slot<G> s(out, cb, b, lane);
    const int64_t left = numel - (int64_t)b * G;
    if (left <= 0) {
      s.zero(lane);
      continue;
    }
    float v[E];
    decode_mean<G>(in, stride, cb, b, W, lane, v);
    const int64_t e0 = (int64_t)b * G + lane * E;
    const bool whole = vec && left >= G;
    uint32_t valid = 0xffffffffu >> (32 - E);
    if (whole) {
      float e[E];
      LaneVec<float, E>::ld(err + e0, e);
#pragma unroll
      for (int k = 0; k < E; ++k) v[k] += e[k];
    } else {
      valid = 0u;
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const bool in = lane * E + k < left;
        v[k] = in ? v[k] + err[e0 + k] : 0.f;
        valid |= in ? 1u << k : 0u;
      }
    }
    compress_block<G>(v, valid, left < G ? (int)left : G, err + e0, whole, s, lane);
  }
}

// ---- host --------------------------------------------------------------------------------------
int cu_count(int device) {
  int v = 0;
  return hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && v > 0 ? v : 256;
}

dim3 grid_for(int64_t blocks, int device) {
  const int64_t groups = (blocks + kOW - 1) / kOW;
  return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(groups, (int64_t)cu_count(device) * kOGroupsPerCU)));
}

void check_block(const char* op, int64_t block, int64_t segments) {
  TORCH_CHECK(block == 512 || block == 1024 || block == 2048, op, ": block must be 512, 1024 or 2048, got ", block);
  TORCH_CHECK(segments >= 1 && segments <= 65536, op, ": segments must be in [1, 65536], got ", segments);
}

void check_payload(const char* op, const char* name, const at::Tensor& p, const at::Device& device) {
  TORCH_CHECK(p.is_cuda() && p.device() == device && p.scalar_type() == at::kByte && p.dim() == 1 &&
                  p.is_contiguous(),
              op, ": ", name, " must be a flat contiguous uint8 tensor on ", device);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(p.data_ptr()) % 4 == 0, op, ": ", name, " must be 4-byte aligned");
}

void check_bucket(const char* op, const char* name, const at::Tensor& t) {
  const auto st = t.scalar_type();
  TORCH_CHECK(t.is_cuda() && t.dim() == 1 && t.is_contiguous() &&
                  (st == at::kFloat || st == at::kBFloat16 || st == at::kHalf),
              op, ": ", name, " must be a flat contiguous fp32 / bf16 / fp16 CUDA tensor");
  TORCH_CHECK(t.numel() < (int64_t(1) << 37), op, ": ", name, " has too many elements");  // blocks fit 32 bits
}

void check_err(const char* op, const at::Tensor& err, int64_t numel, const at::Device& device) {
  TORCH_CHECK(err.is_cuda() && err.device() == device && err.scalar_type() == at::kFloat && err.dim() == 1 &&
                  err.is_contiguous(),
              op, ": err must be a flat contiguous fp32 tensor on ", device);
  TORCH_CHECK(err.numel() == numel, op, ": err must hold ", numel, " elements, got ", err.numel());
}

bool aligned16(const at::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }

#define XDDP_ONEBIT_BLOCK_SWITCH(block, ...)                   \
  switch (block) {                                             \
    case 512: { constexpr int G = 512; __VA_ARGS__; break; }   \
    case 1024: { constexpr int G = 1024; __VA_ARGS__; break; } \
    default: { constexpr int G = 2048; __VA_ARGS__; break; }   \
  }

template <typename T>
void launch_compress(const at::Tensor& x, at::Tensor& err, at::Tensor& payload, int64_t block, unsigned nb,
                     unsigned cb, unsigned total, hipStream_t stream) {
  const dim3 grid = grid_for(total, x.device().index());
  XDDP_ONEBIT_BLOCK_SWITCH(block, hipLaunchKernelGGL((onebit_compress_kernel<T, G>), grid, dim3(kOT), 0, stream,
                                                     reinterpret_cast<const T*>(x.data_ptr()), err.data_ptr<float>(),
                                                     payload.data_ptr<uint8_t>(), x.numel(), nb, cb, total,
                                                     aligned16(x) && aligned16(err) ? 1 : 0));
}

template <typename T>
void launch_decode(const at::Tensor& payload, at::Tensor& out, int64_t block, unsigned nb, unsigned cb, int W,
                   int concat, hipStream_t stream) {
  const dim3 grid = grid_for(nb, out.device().index());
  XDDP_ONEBIT_BLOCK_SWITCH(block, hipLaunchKernelGGL((onebit_decode_kernel<T, G>), grid, dim3(kOT), 0, stream,
                                                     payload.data_ptr<uint8_t>(), reinterpret_cast<T*>(out.data_ptr()),
                                                     out.numel(), nb, cb, W, concat, aligned16(out) ? 1 : 0));
}

}  // namespace

void onebit_compress(const at::Tensor& x, at::Tensor err, at::Tensor payload, int64_t block, int64_t segments) {
  check_block("onebit_compress", block, segments);
  check_bucket("onebit_compress", "x", x);
  check_err("onebit_compress", err, x.numel(), x.device());
  check_payload("onebit_compress", "payload", payload, x.device());
  const int64_t n = x.numel(), nb = (n + block - 1) / block, cb = (nb + segments - 1) / segments;
  const int64_t bpb = block / 8 + 4;
  TORCH_CHECK(payload.numel() == segments * cb * bpb, "onebit_compress: payload must hold ", segments * cb * bpb,
              " bytes (", segments, " segments of ", cb, " blocks), got ", payload.numel());
  TORCH_CHECK(segments * cb < (int64_t(1) << 31), "onebit_compress: too many blocks");
  if (n == 0) return;
  auto stream = c10::hip::getCurrentHIPStream(x.device().index()).stream();
  const unsigned unb = (unsigned)nb, ucb = (unsigned)cb, total = (unsigned)(segments * cb);
  if (x.scalar_type() == at::kFloat) launch_compress<float>(x, err, payload, block, unb, ucb, total, stream);
  else if (x.scalar_type() == at::kBFloat16)
    launch_compress<dev::bf16_t>(x, err, payload, block, unb, ucb, total, stream);
  else launch_compress<dev::f16_t>(x, err, payload, block, unb, ucb, total, stream);
  XDDP_HIP_CHECK(hipGetLastError());
}

void onebit_decode_mean(const at::Tensor& payload, at::Tensor out, int64_t block, int64_t segments,
                        const std::string& mode) {
  check_block("onebit_decode_mean", block, segments);
  TORCH_CHECK(mode == "mean" || mode == "concat", "onebit_decode_mean: mode must be \"mean\" or \"concat\", got \"",
              mode, "\"");
  check_bucket("onebit_decode_mean", "out", out);
  check_payload("onebit_decode_mean", "payload", payload, out.device());
  const bool concat = mode == "concat";
  const int64_t n = out.numel(), nb = (n + block - 1) / block;
  const int64_t cb = concat ? (nb + segments - 1) / segments : nb;
  const int64_t bpb = block / 8 + 4;
  TORCH_CHECK(payload.numel() == segments * cb * bpb, "onebit_decode_mean: payload must hold ", segments * cb * bpb,
              " bytes (", segments, " segments of ", cb, " blocks), got ", payload.numel());
  TORCH_CHECK(segments * cb < (int64_t(1) << 31), "onebit_decode_mean: too many blocks");
  if (n == 0) return;
  auto stream = c10::hip::getCurrentHIPStream(out.device().index()).stream();
  const int W = concat ? 1 : (int)segments;
  const unsigned unb = (unsigned)nb, ucb = (unsigned)cb;
  if (out.scalar_type() == at::kFloat) launch_decode<float>(payload, out, block, unb, ucb, W, concat, stream);
  else if (out.scalar_type() == at::kBFloat16)
    launch_decode<dev::bf16_t>(payload, out, block, unb, ucb, W, concat, stream);
  else launch_decode<dev::f16_t>(payload, out, block, unb, ucb, W, concat, stream);
  XDDP_HIP_CHECK(hipGetLastError());
}

void onebit_reduce_recompress(const at::Tensor& payload_in, at::Tensor err, at::Tensor payload_out, int64_t block,
                              int64_t segments, int64_t numel) {
  check_block("onebit_reduce_recompress", block, segments);
  TORCH_CHECK(payload_in.is_cuda(), "onebit_reduce_recompress: payload_in must be a CUDA tensor");
  check_payload("onebit_reduce_recompress", "payload_in", payload_in, payload_in.device());
  check_payload("onebit_reduce_recompress", "payload_out", payload_out, payload_in.device());
  const int64_t seg = payload_out.numel(), bpb = block / 8 + 4;
  TORCH_CHECK(seg % bpb == 0 && payload_in.numel() == segments * seg,
              "onebit_reduce_recompress: payload_out must hold whole blocks of ", bpb, " bytes and payload_in ",
              segments, " such segments (", segments * seg, " bytes), got ", seg, " and ", payload_in.numel(),
              " bytes");
  const int64_t cb = seg / bpb;
  TORCH_CHECK(cb < (int64_t(1) << 31), "onebit_reduce_recompress: too many blocks");
  check_err("onebit_reduce_recompress", err, cb * block, payload_in.device());
  TORCH_CHECK(numel >= 0 && numel <= cb * block, "onebit_reduce_recompress: numel must be in [0, ", cb * block,
              "], got ", numel);
  if (cb == 0) return;
  auto stream = c10::hip::getCurrentHIPStream(payload_in.device().index()).stream();
  const dim3 grid = grid_for(cb, payload_in.device().index());
  XDDP_ONEBIT_BLOCK_SWITCH(block, hipLaunchKernelGGL((onebit_reduce_recompress_kernel<G>), grid, dim3(kOT), 0, stream,
                                                     payload_in.data_ptr<uint8_t>(), err.data_ptr<float>(),
                                                     payload_out.data_ptr<uint8_t>(), (unsigned)cb, (int)segments,
                                                     numel, aligned16(err) ? 1 : 0));
  XDDP_HIP_CHECK(hipGetLastError());
}

}  // namespace kernels
}  // namespace xddp
