// Multi-tensor HIP kernels for the DDP hot path on gfx950 (CDNA4).
//
// One launch walks a list of up to kMaxSeg tensors described in the kernel-argument
// segment table (no H2D upload, so the launch is graph-capturable). Every block owns a
// fixed 8192-element chunk of one segment; each lane moves 8 elements per iteration with
// 16-byte loads/stores (Guideline 13) and converts dtypes in registers (bf16 through
// v_cvt_pk_bf16_f32). Grids are thousands of blocks for MB-sized buckets, well past the
// 256 CUs.
#include "kernels/multi_tensor.h"

#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "kernels/dev_utils.h"

namespace xddp {
namespace kernels {

using dev::bf16_t;
using dev::f16_t;
using dev::Elem;
using dev::Vec8;

constexpr int kThreads = 256;
constexpr int kIters = 4;
constexpr int64_t kChunk = (int64_t)kThreads * 8 * kIters;  // elements per block
constexpr int kMaxSeg = 40;

template <int NPTR>
struct SegTable {
  void* ptr[NPTR][kMaxSeg];
  int64_t numel[kMaxSeg];
  int32_t blk_end[kMaxSeg];  // inclusive prefix sum of blocks per segment
  int32_t nseg;
};

template <int NPTR>
__device__ __forceinline__ int find_seg(const SegTable<NPTR>& t, int b) {
  // wave-uniform binary search over the (kernarg-resident) prefix array
  int lo = 0, hi = t.nseg - 1;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (b < t.blk_end[mid]) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// What a block of a list kernel works on: segment `s`, its element count and the block's first element
struct Chunk {
  int s;
  int64_t n, base;
};
template <int NPTR>
__device__ __forceinline__ Chunk block_chunk(const SegTable<NPTR>& t) {
  const int s = find_seg(t, blockIdx.x);
  const int64_t blk = blockIdx.x - (s ? t.blk_end[s - 1] : 0);
  return {s, t.numel[s], blk * kChunk};
}
// Builds segment tables and launches `launch(table, nblocks)` whenever one fills.
template <int NPTR, typename F>
static void for_each_table(const std::vector<std::array<void*, NPTR>>& ptrs, const std::vector<int64_t>& numels,
                           F&& launch) {
  SegTable<NPTR> t;
  t.nseg = 0;
  int32_t blocks = 0;
  for (size_t i = 0; i < ptrs.size(); ++i) {
    const int64_t n = numels[i];
    if (n == 0) continue;
    int64_t nb = (n + kChunk - 1) / kChunk;
    TORCH_CHECK(nb < (int64_t)(1 << 30), "tensor too large for multi-tensor launch");
    if (t.nseg == kMaxSeg || (int64_t)blocks + nb > (int64_t)(1 << 30)) {
      launch(t, blocks);
      t.nseg = 0;
      blocks = 0;
    }
    for (int p = 0; p < NPTR; ++p) t.ptr[p][t.nseg] = ptrs[i][p];
    t.numel[t.nseg] = n;
    blocks += (int32_t)nb;
    t.blk_end[t.nseg] = blocks;
    t.nseg++;
  }
  if (t.nseg) launch(t, blocks);
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ------------------------------------------------------------------------------------
// scale-copy: dst = cast(src * scale * (*sp))
// ------------------------------------------------------------------------------------
template <typename Ti, typename To, bool VEC>
__global__ __launch_bounds__(kThreads) void scale_copy_kernel(SegTable<2> t, float scale, const float* sp) {
  const int s = find_seg(t, blockIdx.x);
  const int64_t blk = blockIdx.x - (s ? t.blk_end[s - 1] : 0);
  const Ti* __restrict__ src = reinterpret_cast<const Ti*>(t.ptr[0][s]);
  To* __restrict__ dst = reinterpret_cast<To*>(t.ptr[1][s]);
  const int64_t n = t.numel[s];
  const float sc = sp ? scale * (*sp) : scale;
  const int64_t base = blk * kChunk;
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int64_t i = base + ((int64_t)it * kThreads + threadIdx.x) * 8;
    if (VEC && i + 8 <= n) {
      float v[8];
      Vec8<Ti>::ld(src + i, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] *= sc;
      Vec8<To>::st(dst + i, v);
    } else {
      for (int64_t k = i; k < i + 8 && k < n; ++k)
        Elem<To, float>::st(dst, k, Elem<Ti, float>::ld(src, k) * sc);
    }
  }
}

template <typename Ti, typename To>
__global__ __launch_bounds__(kThreads) void scale_copy_kernel_f64(SegTable<2> t, double scale, const float* sp) {
  const int s = find_seg(t, blockIdx.x);
  const int64_t blk = blockIdx.x - (s ? t.blk_end[s - 1] : 0);
  const Ti* src = reinterpret_cast<const Ti*>(t.ptr[0][s]);
  To* dst = reinterpret_cast<To*>(t.ptr[1][s]);
  const int64_t n = t.numel[s];
  const double sc = sp ? scale * (double)(*sp) : scale;
  for (int64_t k = blk * kChunk + threadIdx.x; k < std::min(n, (blk + 1) * kChunk); k += kThreads)
    Elem<To, double>::st(dst, k, Elem<Ti, double>::ld(src, k) * sc);
}

template <typename T>
struct DevType {
  using type = T;
};
template <>
struct DevType<at::BFloat16> {
  using type = bf16_t;
};
template <>
struct DevType<at::Half> {
  using type = f16_t;
};

#define XDDP_DISPATCH_CASES_F32_BF16_F16(NAME, ...)                  \
    case at::kFloat: { using NAME = float; __VA_ARGS__; break; }     \
    case at::kBFloat16: { using NAME = bf16_t; __VA_ARGS__; break; } \
    case at::kHalf: { using NAME = f16_t; __VA_ARGS__; break; }
#define XDDP_DISPATCH_FLOAT(st, NAME, ...)                                     \
  switch (st) {                                                                \
    XDDP_DISPATCH_CASES_F32_BF16_F16(NAME, __VA_ARGS__)                        \
    case at::kDouble: { using NAME = double; __VA_ARGS__; break; }             \
    default: TORCH_CHECK(false, "xddp multi-tensor: unsupported dtype ", st);  \
  }
// for kernels without an fp64 form; `what` is the error message up to the dtype
#define XDDP_DISPATCH_FLOAT_NO_F64(st, NAME, what, ...)  \
  switch (st) {                                          \
    XDDP_DISPATCH_CASES_F32_BF16_F16(NAME, __VA_ARGS__)  \
    default: TORCH_CHECK(false, what, st);               \
  }

// ------------------------------------------------------------------------------------
// byte-exact copy (any dtype, bit patterns preserved): "numel" is bytes; a block owns
// kChunk bytes, 16 B per lane per iteration when both ends of the segment are aligned.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void copy_bytes_kernel(SegTable<2> t) {
  const int s = find_seg(t, blockIdx.x);
  const int64_t blk = blockIdx.x - (s ? t.blk_end[s - 1] : 0);
  const char* __restrict__ src = reinterpret_cast<const char*>(t.ptr[0][s]);
  char* __restrict__ dst = reinterpret_cast<char*>(t.ptr[1][s]);
  const int64_t n = t.numel[s];
  const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
  constexpr int kIt = kChunk / (kThreads * 16);
  const int64_t base = blk * kChunk;
#pragma unroll
  for (int it = 0; it < kIt; ++it) {
    const int64_t i = base + ((int64_t)it * kThreads + threadIdx.x) * 16;
    if (vec && i + 16 <= n) {
      *reinterpret_cast<uint4*>(dst + i) = *reinterpret_cast<const uint4*>(src + i);
    } else {
      for (int64_t k = i; k < i + 16 && k < n; ++k) dst[k] = src[k];
    }
  }
}

void mt_copy_bytes(const std::vector<const void*>& src, const std::vector<void*>& dst,
                   const std::vector<int64_t>& nbytes, hipStream_t stream) {
  TORCH_CHECK(src.size() == dst.size() && src.size() == nbytes.size(), "copy_bytes: list length mismatch");
  std::vector<std::array<void*, 2>> ptrs;
  for (size_t i = 0; i < src.size(); ++i) ptrs.push_back({const_cast<void*>(src[i]), dst[i]});
  for_each_table<2>(ptrs, nbytes, [&](const SegTable<2>& t, int32_t nb) {
    hipLaunchKernelGGL(copy_bytes_kernel, dim3(nb), dim3(kThreads), 0, stream, t);
    XDDP_HIP_CHECK(hipGetLastError());
  });
}

static void check_dense_pair(const at::Tensor& a, const at::Tensor& b) {
  TORCH_CHECK(a.numel() == b.numel(), "numel mismatch ", a.numel(), " vs ", b.numel());
  TORCH_CHECK(a.is_non_overlapping_and_dense() && b.is_non_overlapping_and_dense(),
              "multi-tensor copy needs dense tensors");
  if (a.dim() > 0 && a.numel() > 1) TORCH_CHECK(a.strides() == b.strides() || (a.is_contiguous() && b.is_contiguous()),
              "multi-tensor copy needs identical memory order");
}

static void launch_scale_copy(const std::vector<std::array<void*, 2>>& ptrs, const std::vector<int64_t>& numels,
                              at::ScalarType ti, at::ScalarType to, double scale, const float* sp,
                              hipStream_t stream) {
  bool vec = true;
  for (auto& p : ptrs) vec = vec && aligned16(p[0]) && aligned16(p[1]);
  const bool f64 = (ti == at::kDouble || to == at::kDouble);
  XDDP_DISPATCH_FLOAT(ti, Ti, XDDP_DISPATCH_FLOAT(to, To, {
    for_each_table<2>(ptrs, numels, [&](const SegTable<2>& t, int32_t nb) {
      if (f64)
        hipLaunchKernelGGL((scale_copy_kernel_f64<Ti, To>), dim3(nb), dim3(kThreads), 0, stream, t, scale, sp);
      else if (vec)
        hipLaunchKernelGGL((scale_copy_kernel<Ti, To, true>), dim3(nb), dim3(kThreads), 0, stream, t, (float)scale, sp);
      else
        hipLaunchKernelGGL((scale_copy_kernel<Ti, To, false>), dim3(nb), dim3(kThreads), 0, stream, t, (float)scale, sp);
      XDDP_HIP_CHECK(hipGetLastError());
    });
  }));
}

static const float* scale_ptr(const c10::optional<at::Tensor>& st) {
  if (!st.has_value() || !st->defined()) return nullptr;
  TORCH_CHECK(st->scalar_type() == at::kFloat && st->is_cuda(), "scale tensor must be a float32 device tensor");
  return st->data_ptr<float>();
}

void mt_scale_copy(const std::vector<at::Tensor>& src, const std::vector<at::Tensor>& dst, double scale,
                   const c10::optional<at::Tensor>& scale_tensor, hipStream_t stream) {
  TORCH_CHECK(src.size() == dst.size(), "src/dst list length mismatch");
  if (src.empty()) return;
  std::vector<std::array<void*, 2>> ptrs;
  std::vector<int64_t> numels;
  ptrs.reserve(src.size());
  numels.reserve(src.size());
  const auto ti = src[0].scalar_type(), to = dst[0].scalar_type();
  for (size_t i = 0; i < src.size(); ++i) {
    TORCH_CHECK(src[i].scalar_type() == ti && dst[i].scalar_type() == to, "mixed dtypes in tensor list");
    TORCH_CHECK(src[i].is_cuda() && dst[i].is_cuda(), "mt_scale_copy expects device tensors");
    check_dense_pair(src[i], dst[i]);
    ptrs.push_back({const_cast<void*>(src[i].data_ptr()), dst[i].data_ptr()});
    numels.push_back(src[i].numel());
  }
  launch_scale_copy(ptrs, numels, ti, to, scale, scale_ptr(scale_tensor), stream);
}

void mt_pack(const std::vector<at::Tensor>& src, const at::Tensor& flat, const std::vector<int64_t>& offsets,
             double scale, hipStream_t stream) {
  TORCH_CHECK(src.size() == offsets.size(), "pack: offsets length mismatch");
  if (src.empty()) return;
  TORCH_CHECK(flat.is_contiguous(), "pack target must be contiguous");
  const auto ti = src[0].scalar_type(), to = flat.scalar_type();
  const int64_t es = flat.element_size();
  std::vector<std::array<void*, 2>> ptrs;
  std::vector<int64_t> numels;
  for (size_t i = 0; i < src.size(); ++i) {
    TORCH_CHECK(src[i].scalar_type() == ti, "mixed dtypes in pack list");
    TORCH_CHECK(src[i].is_non_overlapping_and_dense(), "pack source must be dense");
    TORCH_CHECK(offsets[i] + src[i].numel() <= flat.numel(), "pack overflows target");
    ptrs.push_back({const_cast<void*>(src[i].data_ptr()), static_cast<char*>(flat.data_ptr()) + offsets[i] * es});
    numels.push_back(src[i].numel());
  }
  launch_scale_copy(ptrs, numels, ti, to, scale, nullptr, stream);
}

void mt_unpack(const at::Tensor& flat, const std::vector<int64_t>& offsets, const std::vector<at::Tensor>& dst,
               double scale, hipStream_t stream) {
  TORCH_CHECK(dst.size() == offsets.size(), "unpack: offsets length mismatch");
  if (dst.empty()) return;
  TORCH_CHECK(flat.is_contiguous(), "unpack source must be contiguous");
  const auto ti = flat.scalar_type(), to = dst[0].scalar_type();
  const int64_t es = flat.element_size();
  std::vector<std::array<void*, 2>> ptrs;
  std::vector<int64_t> numels;
  for (size_t i = 0; i < dst.size(); ++i) {
    TORCH_CHECK(dst[i].scalar_type() == to, "mixed dtypes in unpack list");
    TORCH_CHECK(dst[i].is_non_overlapping_and_dense(), "unpack target must be dense");
    TORCH_CHECK(offsets[i] + dst[i].numel() <= flat.numel(), "unpack overflows source");
    ptrs.push_back({static_cast<char*>(flat.data_ptr()) + offsets[i] * es, dst[i].data_ptr()});
    numels.push_back(dst[i].numel());
  }
  launch_scale_copy(ptrs, numels, ti, to, scale, nullptr, stream);
}

// ------------------------------------------------------------------------------------
// L2 norm (deterministic two-pass: per-block partials, then one block folds them)
// ------------------------------------------------------------------------------------
// The type a tensor's elements are read and reduced in: fp32, except fp64 tensors, whose values
// (and squares) may lie outside fp32's range.
template <typename T>
struct Compute {
  using type = float;
};
template <>
struct Compute<double> {
  using type = double;
};

template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void sumsq_kernel(SegTable<1> t, typename Compute<T>::type* partials,
                                                         int32_t part_off) {
  using A = typename Compute<T>::type;
  __shared__ A scratch[kThreads / 64];
  const int s = find_seg(t, blockIdx.x);
  const int64_t blk = blockIdx.x - (s ? t.blk_end[s - 1] : 0);
  const T* x = reinterpret_cast<const T*>(t.ptr[0][s]);
  const int64_t n = t.numel[s];
  const int64_t base = blk * kChunk;
  A acc = 0;
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int64_t i = base + ((int64_t)it * kThreads + threadIdx.x) * 8;
    if (VEC && i + 8 <= n) {
      A v[8];
      Vec8<T>::ld(x + i, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = fma(v[j], v[j], acc);
    } else {
      for (int64_t k = i; k < i + 8 && k < n; ++k) {
        A v = Elem<T, A>::ld(x, k);
        acc = fma(v, v, acc);
      }
    }
  }
  acc = dev::block_sum(acc, scratch);
  if (threadIdx.x == 0) partials[part_off + blockIdx.x] = acc;
}

// out[1] is always written: 1 when there is nothing to clip to (max_norm <= 0)
template <typename A>
__global__ __launch_bounds__(1024) void norm_finalize_kernel(const A* partials, int64_t n, float* out,
                                                             float max_norm) {
  __shared__ A scratch[1024 / 64];
  A acc = 0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) acc += partials[i];
  acc = dev::block_sum(acc, scratch);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(acc);
    out[0] = norm;
    out[1] = max_norm > 0.f ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f;
  }
}

void mt_l2norm(const std::vector<at::Tensor>& tensors, const at::Tensor& out, double max_norm, hipStream_t stream) {
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.numel() >= 2 && out.is_cuda(), "out must be float32[>=2] on device");
  if (tensors.empty()) {
    out.zero_();
    out.narrow(0, 1, 1).fill_(1.0);
    return;
  }
  const auto st = tensors[0].scalar_type();
  std::vector<std::array<void*, 1>> ptrs;
  std::vector<int64_t> numels;
  int64_t total_blocks = 0;
  bool vec = true;
  for (auto& x : tensors) {
    TORCH_CHECK(x.scalar_type() == st, "mixed dtypes in norm list");
    TORCH_CHECK(x.is_non_overlapping_and_dense(), "norm needs dense tensors");
    ptrs.push_back({const_cast<void*>(x.data_ptr())});
    numels.push_back(x.numel());
    total_blocks += (x.numel() + kChunk - 1) / kChunk;
    vec = vec && aligned16(x.data_ptr());
  }
  auto partials = at::empty({std::max<int64_t>(total_blocks, 1)}, out.options().dtype(st == at::kDouble ? at::kDouble : at::kFloat));
  int32_t off = 0;
  XDDP_DISPATCH_FLOAT(st, T, {
    using A = typename Compute<T>::type;
    A* part = partials.data_ptr<A>();
    for_each_table<1>(ptrs, numels, [&](const SegTable<1>& t, int32_t nb) {
      if (vec)
        hipLaunchKernelGGL((sumsq_kernel<T, true>), dim3(nb), dim3(kThreads), 0, stream, t, part, off);
      else
        hipLaunchKernelGGL((sumsq_kernel<T, false>), dim3(nb), dim3(kThreads), 0, stream, t, part, off);
      XDDP_HIP_CHECK(hipGetLastError());
      off += nb;
    });
    hipLaunchKernelGGL(norm_finalize_kernel<A>, dim3(1), dim3(1024), 0, stream, part, (int64_t)off,
                       out.data_ptr<float>(), (float)max_norm);
    XDDP_HIP_CHECK(hipGetLastError());
  });
}

// ------------------------------------------------------------------------------------
// non-finite check (TORCH_NCCL_NAN_CHECK analogue)
// ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void nonfinite_kernel(SegTable<1> t, int* flag) {
  const int s = find_seg(t, blockIdx.x);
  const int64_t blk = blockIdx.x - (s ? t.blk_end[s - 1] : 0);
  const T* x = reinterpret_cast<const T*>(t.ptr[0][s]);
  const int64_t n = t.numel[s];
  bool bad = false;
  for (int64_t k = blk * kChunk + threadIdx.x; k < std::min(n, (blk + 1) * kChunk); k += kThreads) {
    const typename Compute<T>::type v = Elem<T, typename Compute<T>::type>::ld(x, k);  // fp64 tested as fp64
    bad |= !isfinite(v);
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

void mt_nonfinite(const std::vector<at::Tensor>& tensors, const at::Tensor& out, hipStream_t stream) {
  TORCH_CHECK(out.scalar_type() == at::kInt && out.is_cuda(), "flag must be int32 device tensor");
  XDDP_HIP_CHECK(hipMemsetAsync(out.data_ptr(), 0, sizeof(int), stream));
  if (tensors.empty()) return;
  const auto st = tensors[0].scalar_type();
  std::vector<std::array<void*, 1>> ptrs;
  std::vector<int64_t> numels;
  for (auto& x : tensors) {
    TORCH_CHECK(x.scalar_type() == st && x.is_non_overlapping_and_dense(), "nonfinite: dense, single dtype");
    ptrs.push_back({const_cast<void*>(x.data_ptr())});
    numels.push_back(x.numel());
  }
  XDDP_DISPATCH_FLOAT(st, T, {
    for_each_table<1>(ptrs, numels, [&](const SegTable<1>& t, int32_t nb) {
      hipLaunchKernelGGL((nonfinite_kernel<T>), dim3(nb), dim3(kThreads), 0, stream, t, out.data_ptr<int>());
      XDDP_HIP_CHECK(hipGetLastError());
    });
  });
}

// ------------------------------------------------------------------------------------
// replica checksum: fp64 sum of the values + XOR of a 64-bit mix of every element's raw bits with
// its (tensor, index) position, over a list of tensors of any dtypes. Per-block partials are
// written at fixed slots and merged by one block in a fixed order, so equal bytes on two ranks
// give bit-equal checksums (the DDP replica check compares them across ranks).
// ------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {  // splitmix64 finalizer
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
template <typename T>
__device__ __forceinline__ unsigned long long raw_bits(const T* x, int64_t k) {
  if constexpr (sizeof(T) == 8) return reinterpret_cast<const unsigned long long*>(x)[k];
  else if constexpr (sizeof(T) == 4) return reinterpret_cast<const uint32_t*>(x)[k];
  else if constexpr (sizeof(T) == 2) return reinterpret_cast<const uint16_t*>(x)[k];
  else return reinterpret_cast<const uint8_t*>(x)[k];
}
template <typename T>
__device__ __forceinline__ double as_double(const T* x, int64_t k) {
  if constexpr (std::is_same<T, bf16_t>::value || std::is_same<T, f16_t>::value) return (double)Elem<T, float>::ld(x, k);
  else return (double)x[k];
}

template <typename T>
__global__ __launch_bounds__(kThreads) void checksum_kernel(SegTable<2> t, double* psum, unsigned long long* phash,
                                                            int32_t off) {
  __shared__ double ssum[kThreads / 64];
  __shared__ unsigned long long shash[kThreads / 64];
  const int s = find_seg(t, blockIdx.x);
  const int64_t blk = blockIdx.x - (s ? t.blk_end[s - 1] : 0);
  const T* x = reinterpret_cast<const T*>(t.ptr[0][s]);
  const unsigned long long seed = mix64(reinterpret_cast<uintptr_t>(t.ptr[1][s]) + 0x9e3779b97f4a7c15ull);
  const int64_t n = t.numel[s];
  double acc = 0.0;
  unsigned long long h = 0ull;
  const int64_t end = std::min(n, (blk + 1) * kChunk);
  for (int64_t k = blk * kChunk + threadIdx.x; k < end; k += kThreads) {
    acc += as_double(x, k);
    h ^= mix64(raw_bits(x, k) ^ mix64(seed + (unsigned long long)k));
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o, 64);
    h ^= __shfl_xor(h, o, 64);
  }
  if (lane == 0) {
    ssum[wid] = acc;
    shash[wid] = h;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0;
    unsigned long long hh = 0ull;
    for (int w = 0; w < kThreads / 64; ++w) {
      a += ssum[w];
      hh ^= shash[w];
    }
    psum[off + blockIdx.x] = a;
    phash[off + blockIdx.x] = hh;
  }
}

// one block, fixed order: out = [sum, hash low 32 bits, hash high 32 bits] as float64 (exact)
__global__ __launch_bounds__(kThreads) void checksum_finalize_kernel(const double* psum, const unsigned long long* phash,
                                                                     int64_t n, double* out) {
  __shared__ double ssum[kThreads];
  __shared__ unsigned long long shash[kThreads];
  double a = 0.0;
  unsigned long long h = 0ull;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) {
    a += psum[i];
    h ^= phash[i];
  }
  ssum[threadIdx.x] = a;
  shash[threadIdx.x] = h;
  __syncthreads();
  for (int st = kThreads / 2; st > 0; st >>= 1) {
    if (threadIdx.x < st) {
      ssum[threadIdx.x] += ssum[threadIdx.x + st];
      shash[threadIdx.x] ^= shash[threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = ssum[0];
    out[1] = (double)(shash[0] & 0xffffffffull);
    out[2] = (double)(shash[0] >> 32);
  }
}

at::Tensor mt_checksum(const std::vector<at::Tensor>& tensors, hipStream_t stream) {
  TORCH_CHECK(!tensors.empty(), "checksum of an empty tensor list");
  const auto dev = tensors[0].device();
  auto out = at::zeros({3}, at::TensorOptions().dtype(at::kDouble).device(dev));
  int64_t total_blocks = 0;
  for (auto& x : tensors) {
    TORCH_CHECK(x.device() == dev && x.is_non_overlapping_and_dense(), "checksum: dense tensors on one device");
    total_blocks += (x.numel() + kChunk - 1) / kChunk;
  }
  auto psum = at::empty({std::max<int64_t>(total_blocks, 1)}, out.options());
  auto phash = at::empty({std::max<int64_t>(total_blocks, 1)}, out.options().dtype(at::kLong));
  int32_t off = 0;
  // one table per dtype; the tensor's position in the list seeds its mix (order-sensitive)
  std::vector<at::ScalarType> seen;
  for (auto& x0 : tensors)
    if (std::find(seen.begin(), seen.end(), x0.scalar_type()) == seen.end()) seen.push_back(x0.scalar_type());
  for (auto st : seen) {
    std::vector<std::array<void*, 2>> ptrs;
    std::vector<int64_t> numels;
    for (size_t i = 0; i < tensors.size(); ++i) {
      if (tensors[i].scalar_type() != st) continue;
      ptrs.push_back({const_cast<void*>(tensors[i].data_ptr()), reinterpret_cast<void*>((uintptr_t)(i + 1))});
      numels.push_back(tensors[i].numel());
    }
    auto launch = [&](auto tag) {
      using T = decltype(tag);
      for_each_table<2>(ptrs, numels, [&](const SegTable<2>& t, int32_t nb) {
        hipLaunchKernelGGL((checksum_kernel<T>), dim3(nb), dim3(kThreads), 0, stream, t, psum.data_ptr<double>(),
                           reinterpret_cast<unsigned long long*>(phash.data_ptr<int64_t>()), off);
        XDDP_HIP_CHECK(hipGetLastError());
        off += nb;
      });
    };
    switch (st) {
      case at::kFloat: launch(float{}); break;
      case at::kBFloat16: launch(bf16_t{}); break;
      case at::kHalf: launch(f16_t{}); break;
      case at::kDouble: launch(double{}); break;
      case at::kLong: launch(int64_t{}); break;
      case at::kInt: launch(int32_t{}); break;
      case at::kShort: launch(int16_t{}); break;
      case at::kByte: launch(uint8_t{}); break;
      case at::kChar: launch(int8_t{}); break;
      case at::kBool: launch(uint8_t{}); break;
      default: TORCH_CHECK(false, "checksum: unsupported dtype ", st);
    }
  }
  hipLaunchKernelGGL(checksum_finalize_kernel, dim3(1), dim3(kThreads), 0, stream, psum.data_ptr<double>(),
                     reinterpret_cast<const unsigned long long*>(phash.data_ptr<int64_t>()), (int64_t)off,
                     out.data_ptr<double>());
  XDDP_HIP_CHECK(hipGetLastError());
  return out;
}

// ------------------------------------------------------------------------------------
// Fused optimizers. Every kernel takes its hyperparameters in one by-value struct, and every
// variant of an optimizer runs one update function.
// ------------------------------------------------------------------------------------
// Launches `kernel(table, args)` over the list, one launch per segment table.
template <int NPTR, typename K, typename A>
static void launch_list(K kernel, const std::vector<std::array<void*, NPTR>>& ptrs, const std::vector<int64_t>& numels,
                        const A& args, hipStream_t stream) {
  for_each_table<NPTR>(ptrs, numels, [&](const SegTable<NPTR>& t, int32_t nb) {
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(kThreads), 0, stream, t, args);
    XDDP_HIP_CHECK(hipGetLastError());
  });
}

// ------------------------------------------------------------------------------------
// Fused SGD: slots {param, grad, momentum_buf}, or with master weights {fp32 master, grad, fp32
// momentum, low-precision model param}
// ------------------------------------------------------------------------------------
struct SgdArgs {
  float lr, momentum, dampening, wd;
  bool nesterov, maximize, first;
  const float* gs;
};

template <bool MOM>
struct SgdUpdate {
  const SgdArgs& a;
  const float gscale;
  __device__ __forceinline__ explicit SgdUpdate(const SgdArgs& a_)
      : a(a_), gscale((a_.gs ? *a_.gs : 1.f) * (a_.maximize ? -1.f : 1.f)) {}
  // LW (layer-wise, LARS): g' + wd w is multiplied by the tensor's trust ratio `lam` first
  template <bool LW = false>
  __device__ __forceinline__ void operator()(float& pv, float gv, float& bv, float lam = 1.f) const {
    float d = gv * gscale;
    if (a.wd != 0.f) d = fmaf(a.wd, pv, d);
    if (LW) d *= lam;
    if (MOM) {
      bv = a.first ? d : fmaf(a.momentum, bv, (1.f - a.dampening) * d);
      d = a.nesterov ? fmaf(a.momentum, bv, d) : bv;
    }
    pv = fmaf(-a.lr, d, pv);
  }
};

// MASTER: the update reads and writes the fp32 master, and the updated master is rounded into the
// model's param (of type P) in the same pass (no second launch that re-reads the masters).
// LW: one more slot, the last, holds the address of the tensor's trust ratio (fused_lars).
template <typename P, typename G, bool VEC, bool MOM, bool MASTER, bool LW = false>
__global__ __launch_bounds__(kThreads) void sgd_kernel(SegTable<(MASTER ? 4 : 3) + (LW ? 1 : 0)> t, SgdArgs a) {
  using W = std::conditional_t<MASTER, float, P>;  // what the update reads and writes
  const Chunk c = block_chunk(t);
  float lam = 1.f;
  if constexpr (LW) lam = *reinterpret_cast<const float*>(t.ptr[MASTER ? 4 : 3][c.s]);
  W* p = reinterpret_cast<W*>(t.ptr[0][c.s]);
  const G* g = reinterpret_cast<const G*>(t.ptr[1][c.s]);
  float* buf = reinterpret_cast<float*>(t.ptr[2][c.s]);
  P* q = nullptr;
  if constexpr (MASTER) q = reinterpret_cast<P*>(t.ptr[3][c.s]);
  const int64_t n = c.n;
  const SgdUpdate<MOM> upd(a);
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int64_t i = c.base + ((int64_t)it * kThreads + threadIdx.x) * 8;
    if (VEC && i + 8 <= n) {
      float pv[8], gv[8], bv[8];
      Vec8<W>::ld(p + i, pv);
      Vec8<G>::ld(g + i, gv);
      if (MOM && !a.first) Vec8<float>::ld(buf + i, bv);
#pragma unroll
      for (int j = 0; j < 8; ++j) upd.template operator()<LW>(pv[j], gv[j], bv[j], lam);
      Vec8<W>::st(p + i, pv);
      if (MOM) Vec8<float>::st(buf + i, bv);
      if (MASTER) Vec8<P>::st(q + i, pv);
    } else {
      for (int64_t k = i; k < i + 8 && k < n; ++k) {
        float pv = Elem<W, float>::ld(p, k), gv = Elem<G, float>::ld(g, k), bv = 0.f;
        if (MOM && !a.first) bv = buf[k];
        upd.template operator()<LW>(pv, gv, bv, lam);
        Elem<W, float>::st(p, k, pv);
        if (MOM) buf[k] = bv;
        if (MASTER) Elem<P, float>::st(q, k, pv);
      }
    }
  }
}

static SgdArgs sgd_args(double lr, double momentum, double dampening, double weight_decay, bool nesterov,
                        bool maximize, bool first_step, const c10::optional<at::Tensor>& grad_scale) {
  return {(float)lr,  (float)momentum, (float)dampening, (float)weight_decay,
          nesterov,   maximize,        first_step,       scale_ptr(grad_scale)};
}

void fused_sgd_master(const std::vector<at::Tensor>& masters, const std::vector<at::Tensor>& grads,
                      const std::vector<at::Tensor>& momentum_bufs, const std::vector<at::Tensor>& model_params,
                      double lr, double momentum, double dampening, double weight_decay, bool nesterov, bool maximize,
                      bool first_step, const c10::optional<at::Tensor>& grad_scale, hipStream_t stream) {
  TORCH_CHECK(masters.size() == grads.size() && masters.size() == model_params.size(), "SGD list length mismatch");
  const bool mom = momentum != 0.0;
  TORCH_CHECK(!mom || momentum_bufs.size() == masters.size(), "momentum buffers missing");
  if (masters.empty()) return;
  const auto gt = grads[0].scalar_type(), mt = model_params[0].scalar_type();
  std::vector<std::array<void*, 4>> ptrs;
  std::vector<int64_t> numels;
  bool vec = true;
  for (size_t i = 0; i < masters.size(); ++i) {
    TORCH_CHECK(masters[i].scalar_type() == at::kFloat, "master weights must be fp32");
    TORCH_CHECK(grads[i].scalar_type() == gt && model_params[i].scalar_type() == mt, "mixed dtypes in SGD list");
    check_dense_pair(masters[i], grads[i]);
    check_dense_pair(masters[i], model_params[i]);
    void* b = nullptr;
    if (mom) {
      TORCH_CHECK(momentum_bufs[i].scalar_type() == at::kFloat, "momentum buffers must be fp32");
      check_dense_pair(masters[i], momentum_bufs[i]);
      b = momentum_bufs[i].data_ptr();
    }
    vec = vec && aligned16(masters[i].data_ptr()) && aligned16(grads[i].data_ptr()) && (!mom || aligned16(b)) &&
          aligned16(model_params[i].data_ptr());
    ptrs.push_back({masters[i].data_ptr(), const_cast<void*>(grads[i].data_ptr()), b, model_params[i].data_ptr()});
    numels.push_back(masters[i].numel());
  }
  const SgdArgs args = sgd_args(lr, momentum, dampening, weight_decay, nesterov, maximize, first_step, grad_scale);
  TORCH_CHECK(mt == at::kBFloat16 || mt == at::kHalf, "master-weight SGD: model params must be bf16/fp16");
  XDDP_DISPATCH_FLOAT(gt, G, {
    auto go = [&](auto tag) {
      using Mdl = decltype(tag);
      launch_list<4>(vec ? (mom ? sgd_kernel<Mdl, G, true, true, true> : sgd_kernel<Mdl, G, true, false, true>)
                         : (mom ? sgd_kernel<Mdl, G, false, true, true> : sgd_kernel<Mdl, G, false, false, true>),
                     ptrs, numels, args, stream);
    };
    if (mt == at::kBFloat16) go(bf16_t{}); else go(f16_t{});
  });
}

void fused_sgd(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
               const std::vector<at::Tensor>& momentum_bufs, double lr, double momentum, double dampening,
               double weight_decay, bool nesterov, bool maximize, bool first_step,
               const c10::optional<at::Tensor>& grad_scale, hipStream_t stream) {
  TORCH_CHECK(params.size() == grads.size(), "params/grads length mismatch");
  const bool mom = momentum != 0.0;
  TORCH_CHECK(!mom || momentum_bufs.size() == params.size(), "momentum buffers missing");
  if (params.empty()) return;
  const auto pt = params[0].scalar_type(), gt = grads[0].scalar_type();
  std::vector<std::array<void*, 3>> ptrs;
  std::vector<int64_t> numels;
  bool vec = true;
  for (size_t i = 0; i < params.size(); ++i) {
    TORCH_CHECK(params[i].scalar_type() == pt && grads[i].scalar_type() == gt, "mixed dtypes in SGD list");
    check_dense_pair(params[i], grads[i]);
    void* b = nullptr;
    if (mom) {
      TORCH_CHECK(momentum_bufs[i].scalar_type() == at::kFloat, "momentum buffers must be fp32");
      check_dense_pair(params[i], momentum_bufs[i]);
      b = momentum_bufs[i].data_ptr();
    }
    ptrs.push_back({params[i].data_ptr(), const_cast<void*>(grads[i].data_ptr()), b});
    numels.push_back(params[i].numel());
    vec = vec && aligned16(params[i].data_ptr()) && aligned16(grads[i].data_ptr()) && (!mom || aligned16(b));
  }
  const SgdArgs args = sgd_args(lr, momentum, dampening, weight_decay, nesterov, maximize, first_step, grad_scale);
  TORCH_CHECK(pt != at::kDouble && gt != at::kDouble, "fused SGD: fp64 unsupported");
  XDDP_DISPATCH_FLOAT(pt, P, XDDP_DISPATCH_FLOAT(gt, G, {
    launch_list<3>(vec ? (mom ? sgd_kernel<P, G, true, true, false> : sgd_kernel<P, G, true, false, false>)
                       : (mom ? sgd_kernel<P, G, false, true, false> : sgd_kernel<P, G, false, false, false>),
                   ptrs, numels, args, stream);
  }));
}

// ------------------------------------------------------------------------------------
// Fused Adam / AdamW: the update, its hyperparameters and the parameter write that the kernel with
// fp32 moments and the one with 8-bit moments share
// ------------------------------------------------------------------------------------
struct AdamArgs {
  float lr, b1, b2, omb1, omb2, eps, wd, bc1, bc2_sqrt;
  bool decoupled, maximize;
  const float* gs;
};
// ... and what keys the stochastic rounding (the 8-bit moments', the bf16 parameter write's)
struct AdamSrArgs : AdamArgs {
  unsigned long long seed;
  uint32_t step;
};

// The only place where 1 - beta, the bias corrections and sqrt(bc2) are formed. omb1 / omb2 are
// 1 - beta1 / 1 - beta2 formed in fp64: 1.f - b2 from the rounded b2 = 0.999f is 1.3e-5 off, which
// exp_avg_sq and the denominator would carry.
static AdamArgs adam_args(double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                          bool decoupled, bool maximize, const c10::optional<at::Tensor>& grad_scale) {
  const double bc1 = 1.0 - std::pow(beta1, (double)step);
  const double bc2 = 1.0 - std::pow(beta2, (double)step);
  return {(float)lr,  (float)beta1,        (float)beta2,          (float)(1.0 - beta1), (float)(1.0 - beta2),
          (float)eps, (float)weight_decay, (float)bc1,            (float)std::sqrt(bc2), decoupled,
          maximize,   scale_ptr(grad_scale)};
}

struct AdamUpdate {
  const AdamArgs& a;
  const float gscale, step_size;
  __device__ __forceinline__ explicit AdamUpdate(const AdamArgs& a_)
      : a(a_), gscale((a_.gs ? *a_.gs : 1.f) * (a_.maximize ? -1.f : 1.f)), step_size(a_.lr / a_.bc1) {}
  __device__ __forceinline__ void operator()(float& pv, float gv, float& mv, float& vv) const {
    float gg = gv * gscale;
    if (a.wd != 0.f) {
      if (a.decoupled) pv *= (1.f - a.lr * a.wd);
      else gg = fmaf(a.wd, pv, gg);
    }
    mv = fmaf(a.b1, mv, a.omb1 * gg);
    vv = fmaf(a.b2, vv, a.omb2 * gg * gg);
    const float denom = sqrtf(vv) / a.bc2_sqrt + a.eps;
    pv = pv - step_size * mv / denom;
  }
};

__device__ __forceinline__ uint32_t mix32(uint32_t x) {  // 2-round multiply-xorshift finalizer
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  return x ^ (x >> 16);
}

// The hash key of (seed, parameter ordinal, step): its low / high half are the 8-bit moments' km / ks
__device__ __forceinline__ unsigned long long sr_key(unsigned long long seed, unsigned long long ordinal,
                                                     uint32_t step) {
  return mix64(seed ^ mix64((ordinal << 32) | step));
}
// Stochastically rounded bf16 parameter write: its key kp is the splitmix64 output after `key`, a
// third stream.
__device__ __forceinline__ uint32_t sr_param_key(unsigned long long key) {
  return (uint32_t)mix64(key + 0x9e3779b97f4a7c15ull);
}
// bf16 bits of x rounded with the 16 random bits of element index e (within its parameter): the upper
// half of (bits of x) + r, i.e. away from zero with probability (discarded bits) / 65536. A sum with
// an all-ones exponent falls back to the upper half of x (a finite x saturates instead of becoming
// inf, +-inf stay); NaN gives the quiet NaN 0x7fc0.
__device__ __forceinline__ uint32_t sr_bf16(float x, int64_t e, uint32_t kp) {
  const uint32_t u = __float_as_uint(x);
  const uint32_t r = mix32((uint32_t)e ^ kp ^ ((uint32_t)((uint64_t)e >> 32) * 0x9e3779b9u)) >> 16;
  uint32_t t = u + r;
  if ((t & 0x7f800000u) == 0x7f800000u) t = u;
  if ((u & 0x7fffffffu) > 0x7f800000u) t = 0x7fc00000u;
  return t >> 16;
}
// 8 consecutive elements from index e0 on, one 16-byte store
__device__ __forceinline__ void st8_sr_bf16(bf16_t* p, const float (&v)[8], int64_t e0, uint32_t kp) {
  dev::u32x4 a;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    a[j] = sr_bf16(v[2 * j], e0 + 2 * j, kp) | (sr_bf16(v[2 * j + 1], e0 + 2 * j + 1, kp) << 16);
  *reinterpret_cast<dev::u32x4*>(p) = a;
}

// How an Adam kernel writes the updated parameter: rounded to nearest in P, or (SR: bf16 parameters
// without a master) with sr_bf16. The random bits hang on the element's index within its parameter
// (`eoff` is that of the range's first element), so any slicing gives the bits of the
// whole-parameter update.
template <typename P, bool SR>
struct ParamWriter {
  static_assert(!SR || std::is_same<P, bf16_t>::value, "stochastic rounding: bf16 parameters");
  P* p;
  int64_t eoff;
  uint32_t kp;
  // the 8 elements from range index i on (16-byte store), and element k alone
  __device__ __forceinline__ void st8(int64_t i, const float (&pv)[8]) const {
    if constexpr (SR) st8_sr_bf16(p + i, pv, eoff + i, kp);
    else Vec8<P>::st(p + i, pv);
  }
  __device__ __forceinline__ void st(int64_t k, float pv) const {
    if constexpr (SR) p[k].x = (uint16_t)sr_bf16(pv, eoff + k, kp);
    else Elem<P, float>::st(p, k, pv);
  }
};

// Validates the lists of one Adam launch (lengths are the caller's): every tensor on the device, one
// dtype per list (fp32 for `states` and `masters`), each dense in its parameter's memory order, and
// ordinals / offsets (where the launch has them) in range.
static void check_adam_lists(const char* who, const std::vector<at::Tensor>& params,
                             const std::vector<at::Tensor>& grads,
                             std::initializer_list<const std::vector<at::Tensor>*> states,
                             const std::vector<at::Tensor>& masters, const std::vector<int64_t>* ordinals,
                             const std::vector<int64_t>* offsets) {
  const auto pt = params[0].scalar_type(), gt = grads[0].scalar_type();
  for (size_t i = 0; i < params.size(); ++i) {
    const at::Tensor& p = params[i];
    TORCH_CHECK(p.is_cuda() && grads[i].is_cuda() && p.scalar_type() == pt && grads[i].scalar_type() == gt, who,
                ": device tensors of one dtype per list expected");
    check_dense_pair(p, grads[i]);
    for (const auto* list : states) {
      const at::Tensor& x = (*list)[i];
      TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat, who, ": Adam states must be fp32 device tensors");
      check_dense_pair(p, x);
    }
    if (!masters.empty()) {
      TORCH_CHECK(masters[i].is_cuda() && masters[i].scalar_type() == at::kFloat, "master weights must be fp32");
      check_dense_pair(p, masters[i]);
    }
    TORCH_CHECK(!ordinals || ((*ordinals)[i] >= 0 && (*ordinals)[i] <= (int64_t)UINT32_MAX && (*offsets)[i] >= 0),
                who, ": bad parameter ordinal or offset");
  }
}

// ------------------------------------------------------------------------------------
// Fused Adam / AdamW with fp32 moments: slots {param, grad, exp_avg, exp_avg_sq, master}, or, for
// stochastically rounded bf16 parameters (SR: no master), {param, grad, exp_avg, exp_avg_sq,
// parameter ordinal, element offset of the range within its parameter}
// ------------------------------------------------------------------------------------
template <typename P, typename G, bool VEC, bool MASTER, bool SR = false>
__global__ __launch_bounds__(kThreads) void adam_kernel(SegTable<SR ? 6 : 5> t,
                                                        std::conditional_t<SR, AdamSrArgs, AdamArgs> a) {
  static_assert(!SR || !MASTER, "stochastic rounding: no master");
  const Chunk c = block_chunk(t);
  P* p = reinterpret_cast<P*>(t.ptr[0][c.s]);
  const G* g = reinterpret_cast<const G*>(t.ptr[1][c.s]);
  float* m = reinterpret_cast<float*>(t.ptr[2][c.s]);
  float* v = reinterpret_cast<float*>(t.ptr[3][c.s]);
  float* mp = nullptr;
  ParamWriter<P, SR> w{p, 0, 0u};
  if constexpr (SR) {
    w.eoff = (int64_t)reinterpret_cast<uintptr_t>(t.ptr[5][c.s]);
    w.kp = sr_param_key(sr_key(a.seed, reinterpret_cast<uintptr_t>(t.ptr[4][c.s]), a.step));
  } else {
    mp = reinterpret_cast<float*>(t.ptr[4][c.s]);
  }
  const int64_t n = c.n;
  const AdamUpdate upd(a);
  if (VEC && c.base + kChunk <= n) {
    // whole chunk: every iteration's loads first, then the updates and stores. (Interleaved, the
    // stores of iteration it may alias the loads of it + 1 for the compiler, so each iteration's 7
    // loads waited alone: 112 B in flight per thread instead of 448 B.)
    float pv[kIters][8], gv[kIters][8], mv[kIters][8], vv[kIters][8];
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int64_t i = c.base + ((int64_t)it * kThreads + threadIdx.x) * 8;
      if (MASTER) Vec8<float>::ld(mp + i, pv[it]); else Vec8<P>::ld(p + i, pv[it]);
      Vec8<G>::ld(g + i, gv[it]);
      Vec8<float>::ld(m + i, mv[it]);
      Vec8<float>::ld(v + i, vv[it]);
    }
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int64_t i = c.base + ((int64_t)it * kThreads + threadIdx.x) * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) upd(pv[it][j], gv[it][j], mv[it][j], vv[it][j]);
      w.st8(i, pv[it]);
      if (MASTER) Vec8<float>::st(mp + i, pv[it]);
      Vec8<float>::st(m + i, mv[it]);
      Vec8<float>::st(v + i, vv[it]);
    }
    return;
  }
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int64_t i = c.base + ((int64_t)it * kThreads + threadIdx.x) * 8;
    if (VEC && i + 8 <= n) {
      float pv[8], gv[8], mv[8], vv[8];
      if (MASTER) Vec8<float>::ld(mp + i, pv); else Vec8<P>::ld(p + i, pv);
      Vec8<G>::ld(g + i, gv);
      Vec8<float>::ld(m + i, mv);
      Vec8<float>::ld(v + i, vv);
#pragma unroll
      for (int j = 0; j < 8; ++j) upd(pv[j], gv[j], mv[j], vv[j]);
      w.st8(i, pv);
      if (MASTER) Vec8<float>::st(mp + i, pv);
      Vec8<float>::st(m + i, mv);
      Vec8<float>::st(v + i, vv);
    } else {
      for (int64_t k = i; k < i + 8 && k < n; ++k) {
        float pv = MASTER ? mp[k] : Elem<P, float>::ld(p, k);
        float gv = Elem<G, float>::ld(g, k), mv = m[k], vv = v[k];
        upd(pv, gv, mv, vv);
        w.st(k, pv);
        if (MASTER) mp[k] = pv;
        m[k] = mv;
        v[k] = vv;
      }
    }
  }
}

void fused_adam(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                const std::vector<at::Tensor>& exp_avgs, const std::vector<at::Tensor>& exp_avg_sqs,
                const std::vector<at::Tensor>& masters, double lr, double beta1, double beta2, double eps,
                double weight_decay, int64_t step, bool decoupled, bool maximize,
                const c10::optional<at::Tensor>& grad_scale, hipStream_t stream) {
  const size_t N = params.size();
  TORCH_CHECK(grads.size() == N && exp_avgs.size() == N && exp_avg_sqs.size() == N, "adam: list length mismatch");
  const bool has_master = !masters.empty();
  TORCH_CHECK(!has_master || masters.size() == N, "adam: masters length mismatch");
  if (N == 0) return;
  TORCH_CHECK(step >= 1, "adam: step must be >= 1");
  const auto pt = params[0].scalar_type(), gt = grads[0].scalar_type();
  TORCH_CHECK(pt != at::kDouble && gt != at::kDouble, "fused Adam: fp64 unsupported");
  check_adam_lists("adam", params, grads, {&exp_avgs, &exp_avg_sqs}, masters, nullptr, nullptr);
  std::vector<std::array<void*, 5>> ptrs;
  std::vector<int64_t> numels;
  bool vec = true;
  for (size_t i = 0; i < N; ++i) {
    ptrs.push_back({params[i].data_ptr(), const_cast<void*>(grads[i].data_ptr()), exp_avgs[i].data_ptr(),
                    exp_avg_sqs[i].data_ptr(), has_master ? masters[i].data_ptr() : nullptr});
    numels.push_back(params[i].numel());
    for (auto* q : ptrs.back()) vec = vec && aligned16(q);
  }
  const AdamArgs args = adam_args(lr, beta1, beta2, eps, weight_decay, step, decoupled, maximize, grad_scale);
  XDDP_DISPATCH_FLOAT(pt, P, XDDP_DISPATCH_FLOAT(gt, G, {
    launch_list<5>(vec ? (has_master ? adam_kernel<P, G, true, true> : adam_kernel<P, G, true, false>)
                       : (has_master ? adam_kernel<P, G, false, true> : adam_kernel<P, G, false, false>),
                   ptrs, numels, args, stream);
  }));
}

// Fused Adam / AdamW with fp32 moments and stochastically rounded bf16 parameters (no fp32 master)
void fused_adam_sr(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                   const std::vector<at::Tensor>& exp_avgs, const std::vector<at::Tensor>& exp_avg_sqs,
                   const std::vector<int64_t>& ordinals, const std::vector<int64_t>& offsets, double lr, double beta1,
                   double beta2, double eps, double weight_decay, int64_t step, int64_t seed, bool decoupled,
                   bool maximize, const c10::optional<at::Tensor>& grad_scale, hipStream_t stream) {
  const char* who = "adam (stochastic rounding)";
  const size_t N = params.size();
  TORCH_CHECK(grads.size() == N && exp_avgs.size() == N && exp_avg_sqs.size() == N && ordinals.size() == N &&
                  offsets.size() == N,
              who, ": list length mismatch");
  if (N == 0) return;
  TORCH_CHECK(step >= 1 && step <= (int64_t)UINT32_MAX && seed >= 0, who, ": step must be in [1, 2^32), seed >= 0");
  TORCH_CHECK(params[0].scalar_type() == at::kBFloat16, who, ": bf16 parameters expected");
  check_adam_lists(who, params, grads, {&exp_avgs, &exp_avg_sqs}, {}, &ordinals, &offsets);
  std::vector<std::array<void*, 6>> ptrs;
  std::vector<int64_t> numels;
  bool vec = true;
  for (size_t i = 0; i < N; ++i) {
    ptrs.push_back({params[i].data_ptr(), const_cast<void*>(grads[i].data_ptr()), exp_avgs[i].data_ptr(),
                    exp_avg_sqs[i].data_ptr(), reinterpret_cast<void*>((uintptr_t)ordinals[i]),
                    reinterpret_cast<void*>((uintptr_t)offsets[i])});
    numels.push_back(params[i].numel());
    for (int q = 0; q < 4; ++q) vec = vec && aligned16(ptrs.back()[q]);
  }
  const AdamSrArgs args = {adam_args(lr, beta1, beta2, eps, weight_decay, step, decoupled, maximize, grad_scale),
                           (unsigned long long)seed, (uint32_t)step};
  XDDP_DISPATCH_FLOAT_NO_F64(grads[0].scalar_type(), G, "fused Adam (stochastic rounding): unsupported gradient dtype ", {
    launch_list<6>(vec ? adam_kernel<bf16_t, G, true, false, true> : adam_kernel<bf16_t, G, false, false, true>,
                   ptrs, numels, args, stream);
  });
}

// ------------------------------------------------------------------------------------
// Fused Adam / AdamW with 8-bit moments: slots {param, grad, m codes, m scales, s codes, s scales,
// master, parameter ordinal, element offset of the range within its parameter}
//
// Both moments are OCP e4m3 codes with one fp32 scale per group of 128 consecutive elements
// (scale = group max / 448); the second moment is stored as s = sqrt(v). A block's 8192-element chunk
// is 64 whole groups, and a group is 16 adjacent lanes x 8 elements, so the two group maxima are
// reduced over a DPP row (no LDS, no barrier). The update itself is AdamUpdate, on the dequantised
// fp32 moments; the parameter uses the fresh fp32 moments, which are re-quantised afterwards with
// stochastic rounding (v_cvt_sr_fp8_f32). The random bits are a stateless hash of (seed, parameter
// ordinal, step, element index within the parameter, moment), so they do not depend on the launch,
// the segment table, the load path or on slicing. Loads and stores differ between the vector path,
// the tail and the unaligned path; everything in between is one function.
// ------------------------------------------------------------------------------------
constexpr int kQGroup = 128;
constexpr float kE4M3Max = 448.f;
static_assert(kChunk % kQGroup == 0 && kQGroup == 16 * 8, "a group is one DPP row of 8-element lanes");
static_assert(sizeof(SegTable<9>) + 128 <= 4096, "the by-value segment table must fit the kernarg segment");

template <int CTRL>
__device__ __forceinline__ float dpp_max(float v) {
  return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true)));
}
// max over the 16 lanes of a DPP row, result in every lane (inputs are >= 0)
__device__ __forceinline__ float row16_max(float v) {
  v = dpp_max<0xB1>(v);   // quad_perm:[1,0,3,2]
  v = dpp_max<0x4E>(v);   // quad_perm:[2,3,0,1]
  v = dpp_max<0x141>(v);  // row_half_mirror
  return dpp_max<0x140>(v);  // row_mirror
}

__device__ __forceinline__ void e4m3x4_decode(uint32_t w, float* f) {
  f[0] = __builtin_amdgcn_cvt_f32_fp8((int)w, 0);
  f[1] = __builtin_amdgcn_cvt_f32_fp8((int)w, 1);
  f[2] = __builtin_amdgcn_cvt_f32_fp8((int)w, 2);
  f[3] = __builtin_amdgcn_cvt_f32_fp8((int)w, 3);
}
// four stochastically rounded e4m3 codes of q[0..3] (already within +-448), random words r[0..3]
__device__ __forceinline__ uint32_t e4m3x4_sr(const float* q, const uint32_t* r) {
  int w = 0;
  w = __builtin_amdgcn_cvt_sr_fp8_f32(q[0], (int)r[0], w, 0);
  w = __builtin_amdgcn_cvt_sr_fp8_f32(q[1], (int)r[1], w, 1);
  w = __builtin_amdgcn_cvt_sr_fp8_f32(q[2], (int)r[2], w, 2);
  w = __builtin_amdgcn_cvt_sr_fp8_f32(q[3], (int)r[3], w, 3);
  return (uint32_t)w;
}

// Re-quantise one lane's 8 fresh moments (m, s = sqrt(v); zeros past the end of the range). `idx` is
// the first element's index within its parameter, km / ks the two moments' hash keys.
__device__ __forceinline__ void adam8_quantize(const float (&m)[8], const float (&sv)[8], int64_t idx, uint32_t km,
                                               uint32_t ks, uint32_t (&mq)[2], uint32_t (&sq)[2], float& msc,
                                               float& ssc) {
  float am = 0.f, as = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    am = fmaxf(am, fabsf(m[j]));
    as = fmaxf(as, sv[j]);
  }
  msc = row16_max(am) / kE4M3Max;
  ssc = row16_max(as) / kE4M3Max;
  // (a scale below the smallest normal float, |m| < 5.3e-36, has no finite inverse: such a group
  // keeps its scale and gets zero codes; s = sqrt(v) >= 3.7e-23 never comes near it)
  const float im = msc >= 1.17549435e-38f ? 1.f / msc : 0.f;
  const float is = ssc >= 1.17549435e-38f ? 1.f / ssc : 0.f;
  const uint32_t lo = (uint32_t)idx, hi = (uint32_t)((uint64_t)idx >> 32) * 0x9e3779b9u;
  float qm[8], qs[8];
  uint32_t rm[8], rs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    qm[j] = fminf(fmaxf(m[j] * im, -kE4M3Max), kE4M3Max);
    qs[j] = fminf(sv[j] * is, kE4M3Max);
    rm[j] = mix32((lo + j) ^ km ^ hi);
    rs[j] = mix32((lo + j) ^ ks ^ hi);
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    mq[h] = e4m3x4_sr(qm + 4 * h, rm + 4 * h);
    uint32_t w = e4m3x4_sr(qs + 4 * h, rs + 4 * h);
    // a live element never gets code 0 (it would reach m / (0 + eps)): up to the smallest code
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (sv[4 * h + b] > 0.f && ((w >> (8 * b)) & 0xffu) == 0u) w |= 1u << (8 * b);
    sq[h] = w;
  }
}

// SR: bf16 parameters without a master, written with sr_bf16 (keyed like the moments, third stream).
template <typename P, typename G, bool VEC, bool MASTER, bool SR = false>
__global__ __launch_bounds__(kThreads) void adam8_kernel(SegTable<9> t, float lr, float b1, float b2, float omb1,
                                                         float omb2, float eps, float wd, float bc1, float bc2_sqrt,
                                                         bool decoupled, bool maximize, const float* gs,
                                                         unsigned long long seed, uint32_t step) {
  static_assert(!SR || !MASTER, "stochastic rounding: no master");
  // (the hyperparameters one by one: taken as the struct, this kernel's vector instantiations came out with other
  // code for the flags and measured 0.3 % slower, profiles/r11_multi_tensor_refactor.txt)
  const AdamSrArgs a = {{lr, b1, b2, omb1, omb2, eps, wd, bc1, bc2_sqrt, decoupled, maximize, gs}, seed, step};
  const Chunk c = block_chunk(t);
  P* p = reinterpret_cast<P*>(t.ptr[0][c.s]);
  const G* g = reinterpret_cast<const G*>(t.ptr[1][c.s]);
  uint8_t* mqp = reinterpret_cast<uint8_t*>(t.ptr[2][c.s]);
  float* msp = reinterpret_cast<float*>(t.ptr[3][c.s]);
  uint8_t* sqp = reinterpret_cast<uint8_t*>(t.ptr[4][c.s]);
  float* ssp = reinterpret_cast<float*>(t.ptr[5][c.s]);
  float* mp = reinterpret_cast<float*>(t.ptr[6][c.s]);
  const int64_t eoff = (int64_t)reinterpret_cast<uintptr_t>(t.ptr[8][c.s]);
  const int64_t n = c.n;
  const unsigned long long key = sr_key(a.seed, reinterpret_cast<uintptr_t>(t.ptr[7][c.s]), a.step);
  const uint32_t km = (uint32_t)key, ks = (uint32_t)(key >> 32);
  const ParamWriter<P, SR> w{p, eoff, SR ? sr_param_key(key) : 0u};
  const AdamUpdate upd(a);
  const int64_t base = c.base;
  const bool lead = (threadIdx.x & 15) == 0;  // the lane that writes its group's two scales
  // dequantise, update, re-quantise one lane's 8 elements, the first `nv` of which exist
  auto update8 = [&](int64_t i, int nv, float (&pv)[8], const float (&gv)[8], uint32_t (&mq)[2], uint32_t (&sq)[2],
                     float& msc, float& ssc) {
    float m[8], sv[8];
    e4m3x4_decode(mq[0], m);
    e4m3x4_decode(mq[1], m + 4);
    e4m3x4_decode(sq[0], sv);
    e4m3x4_decode(sq[1], sv + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float mv = m[j] * msc, sh = sv[j] * ssc;
      float vv = sh * sh;
      upd(pv[j], gv[j], mv, vv);
      m[j] = j < nv ? mv : 0.f;
      sv[j] = j < nv ? sqrtf(vv) : 0.f;
    }
    adam8_quantize(m, sv, eoff + i, km, ks, mq, sq, msc, ssc);
  };
  if (VEC && base + kChunk <= n) {
    // whole chunk: every iteration's loads first, then the updates and stores (as adam_kernel)
    float pv[kIters][8], gv[kIters][8], msc[kIters], ssc[kIters];
    uint32_t mq[kIters][2], sq[kIters][2];
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int64_t i = base + ((int64_t)it * kThreads + threadIdx.x) * 8;
      if (MASTER) Vec8<float>::ld(mp + i, pv[it]); else Vec8<P>::ld(p + i, pv[it]);
      Vec8<G>::ld(g + i, gv[it]);
      const uint2 cm = *reinterpret_cast<const uint2*>(mqp + i), cs = *reinterpret_cast<const uint2*>(sqp + i);
      mq[it][0] = cm.x; mq[it][1] = cm.y;
      sq[it][0] = cs.x; sq[it][1] = cs.y;
      msc[it] = msp[i / kQGroup];
      ssc[it] = ssp[i / kQGroup];
    }
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int64_t i = base + ((int64_t)it * kThreads + threadIdx.x) * 8;
      update8(i, 8, pv[it], gv[it], mq[it], sq[it], msc[it], ssc[it]);
      w.st8(i, pv[it]);
      if (MASTER) Vec8<float>::st(mp + i, pv[it]);
      *reinterpret_cast<uint2*>(mqp + i) = make_uint2(mq[it][0], mq[it][1]);
      *reinterpret_cast<uint2*>(sqp + i) = make_uint2(sq[it][0], sq[it][1]);
      if (lead) {
        msp[i / kQGroup] = msc[it];
        ssp[i / kQGroup] = ssc[it];
      }
    }
    return;
  }
  // the range's last chunk, or unaligned pointers. Every lane runs every iteration, also past the
  // end (with zeros), so the row reductions always see 16 live lanes.
#pragma unroll 1
  for (int it = 0; it < kIters; ++it) {
    const int64_t i = base + ((int64_t)it * kThreads + threadIdx.x) * 8;
    const int nv = (int)std::min<int64_t>(std::max<int64_t>(n - i, 0), 8);
    const int64_t grp = i / kQGroup;
    const bool live = grp * kQGroup < n;  // the group has at least one element
    float pv[8], gv[8], msc = 0.f, ssc = 0.f;
    uint32_t mq[2] = {0u, 0u}, sq[2] = {0u, 0u};
    if (VEC && nv == 8) {
      if (MASTER) Vec8<float>::ld(mp + i, pv); else Vec8<P>::ld(p + i, pv);
      Vec8<G>::ld(g + i, gv);
      const uint2 cm = *reinterpret_cast<const uint2*>(mqp + i), cs = *reinterpret_cast<const uint2*>(sqp + i);
      mq[0] = cm.x; mq[1] = cm.y;
      sq[0] = cs.x; sq[1] = cs.y;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        pv[j] = gv[j] = 0.f;
        if (j < nv) {
          pv[j] = MASTER ? mp[i + j] : Elem<P, float>::ld(p, i + j);
          gv[j] = Elem<G, float>::ld(g, i + j);
          mq[j >> 2] |= (uint32_t)mqp[i + j] << (8 * (j & 3));
          sq[j >> 2] |= (uint32_t)sqp[i + j] << (8 * (j & 3));
        }
      }
    }
    if (live) {
      msc = msp[grp];
      ssc = ssp[grp];
    }
    update8(i, nv, pv, gv, mq, sq, msc, ssc);
    if (VEC && nv == 8) {
      w.st8(i, pv);
      if (MASTER) Vec8<float>::st(mp + i, pv);
      *reinterpret_cast<uint2*>(mqp + i) = make_uint2(mq[0], mq[1]);
      *reinterpret_cast<uint2*>(sqp + i) = make_uint2(sq[0], sq[1]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (j < nv) {
          w.st(i + j, pv[j]);
          if (MASTER) mp[i + j] = pv[j];
          mqp[i + j] = (uint8_t)(mq[j >> 2] >> (8 * (j & 3)));
          sqp[i + j] = (uint8_t)(sq[j >> 2] >> (8 * (j & 3)));
        }
      }
    }
    if (lead && live) {
      msp[grp] = msc;
      ssp[grp] = ssc;
    }
  }
}

void fused_adam8(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                 const std::vector<at::Tensor>& m_q, const std::vector<at::Tensor>& m_scale,
                 const std::vector<at::Tensor>& s_q, const std::vector<at::Tensor>& s_scale,
                 const std::vector<at::Tensor>& masters, const std::vector<int64_t>& ordinals,
                 const std::vector<int64_t>& group_offsets, double lr, double beta1, double beta2, double eps,
                 double weight_decay, int64_t step, int64_t seed, bool decoupled, bool maximize,
                 const c10::optional<at::Tensor>& grad_scale, bool stochastic_params, hipStream_t stream) {
  const size_t N = params.size();
  TORCH_CHECK(grads.size() == N && m_q.size() == N && m_scale.size() == N && s_q.size() == N && s_scale.size() == N &&
                  ordinals.size() == N && group_offsets.size() == N,
              "adam8: list length mismatch");
  const bool has_master = !masters.empty();
  TORCH_CHECK(!has_master || masters.size() == N, "adam8: masters length mismatch");
  if (N == 0) return;
  TORCH_CHECK(step >= 1 && step <= (int64_t)UINT32_MAX, "adam8: step must be in [1, 2^32)");
  const auto pt = params[0].scalar_type(), gt = grads[0].scalar_type();
  TORCH_CHECK(pt != at::kDouble && gt != at::kDouble, "fused Adam: fp64 unsupported");
  TORCH_CHECK(!stochastic_params || (pt == at::kBFloat16 && !has_master),
              "adam8: stochastic parameter rounding is for bf16 parameters without master weights");
  check_adam_lists("adam8", params, grads, {}, masters, &ordinals, &group_offsets);
  std::vector<std::array<void*, 9>> ptrs;
  std::vector<int64_t> numels;
  bool vec = true;
  for (size_t i = 0; i < N; ++i) {
    const int64_t n = params[i].numel(), ng = (n + kQGroup - 1) / kQGroup;
    for (const at::Tensor* q : {&m_q[i], &s_q[i]})
      TORCH_CHECK(q->is_cuda() && q->scalar_type() == at::kByte && q->is_contiguous() && q->numel() == n,
                  "adam8: moment codes must be contiguous uint8 device tensors of the parameter's numel");
    for (const at::Tensor* q : {&m_scale[i], &s_scale[i]})
      TORCH_CHECK(q->is_cuda() && q->scalar_type() == at::kFloat && q->is_contiguous() && q->numel() == ng,
                  "adam8: moment scales must be contiguous fp32 device tensors, one entry per 128 elements");
    void* mp = has_master ? masters[i].data_ptr() : nullptr;
    ptrs.push_back({params[i].data_ptr(), const_cast<void*>(grads[i].data_ptr()), m_q[i].data_ptr(),
                    m_scale[i].data_ptr(), s_q[i].data_ptr(), s_scale[i].data_ptr(), mp,
                    reinterpret_cast<void*>((uintptr_t)ordinals[i]),
                    reinterpret_cast<void*>((uintptr_t)(group_offsets[i] * kQGroup))});
    numels.push_back(n);
    vec = vec && aligned16(params[i].data_ptr()) && aligned16(grads[i].data_ptr()) && aligned16(mp) &&
          (reinterpret_cast<uintptr_t>(m_q[i].data_ptr()) & 7u) == 0 &&
          (reinterpret_cast<uintptr_t>(s_q[i].data_ptr()) & 7u) == 0;
  }
  const AdamArgs a = adam_args(lr, beta1, beta2, eps, weight_decay, step, decoupled, maximize, grad_scale);
  auto launch = [&](auto k) {
    for_each_table<9>(ptrs, numels, [&](const SegTable<9>& t, int32_t nb) {
      hipLaunchKernelGGL(k, dim3(nb), dim3(kThreads), 0, stream, t, a.lr, a.b1, a.b2, a.omb1, a.omb2, a.eps, a.wd,
                         a.bc1, a.bc2_sqrt, a.decoupled, a.maximize, a.gs, (unsigned long long)seed, (uint32_t)step);
      XDDP_HIP_CHECK(hipGetLastError());
    });
  };
  // (no fp64 instantiations: the dtype check above has already refused them)
  const char* bad = "fused Adam (8-bit states): unsupported dtype ";
  if (stochastic_params) {
    XDDP_DISPATCH_FLOAT_NO_F64(gt, G, bad, {
      launch(vec ? adam8_kernel<bf16_t, G, true, false, true> : adam8_kernel<bf16_t, G, false, false, true>);
    });
  } else {
    XDDP_DISPATCH_FLOAT_NO_F64(pt, P, bad, XDDP_DISPATCH_FLOAT_NO_F64(gt, G, bad, {
      launch(vec ? (has_master ? adam8_kernel<P, G, true, true> : adam8_kernel<P, G, true, false>)
                 : (has_master ? adam8_kernel<P, G, false, true> : adam8_kernel<P, G, false, false>));
    }));
  }
}

// ------------------------------------------------------------------------------------
// The stochastic rounding alone: fp32 -> bf16 with sr_bf16, keyed like the optimizers' parameter write
// ------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kThreads) void sr_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ out,
                                                           int64_t n, unsigned long long seed,
                                                           unsigned long long ordinal, uint32_t step, int64_t eoff) {
  const uint32_t kp = sr_param_key(sr_key(seed, ordinal, step));
  const int64_t base = (int64_t)blockIdx.x * kChunk;
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int64_t i = base + ((int64_t)it * kThreads + threadIdx.x) * 8;
    if (VEC && i + 8 <= n) {
      float v[8];
      Vec8<float>::ld(x + i, v);
      st8_sr_bf16(out + i, v, eoff + i, kp);
    } else {
      for (int64_t k = i; k < i + 8 && k < n; ++k) out[k].x = (uint16_t)sr_bf16(x[k], eoff + k, kp);
    }
  }
}

void stochastic_round_bf16(const at::Tensor& x, const at::Tensor& out, int64_t seed, int64_t ordinal, int64_t step,
                           int64_t offset, hipStream_t stream) {
  TORCH_CHECK(x.is_cuda() && out.is_cuda() && x.scalar_type() == at::kFloat && out.scalar_type() == at::kBFloat16,
              "stochastic_round_bf16: float32 input and bfloat16 output on the device expected");
  check_dense_pair(x, out);
  TORCH_CHECK(seed >= 0 && ordinal >= 0 && ordinal <= (int64_t)UINT32_MAX && step >= 0 &&
                  step <= (int64_t)UINT32_MAX && offset >= 0,
              "stochastic_round_bf16: bad seed, ordinal, step or offset");
  const int64_t n = x.numel();
  if (n == 0) return;
  const int64_t nb = (n + kChunk - 1) / kChunk;
  TORCH_CHECK(nb < (int64_t)(1 << 30), "tensor too large for one launch");
  const bool vec = aligned16(x.data_ptr()) && aligned16(out.data_ptr());
  auto k = vec ? sr_bf16_kernel<true> : sr_bf16_kernel<false>;
  hipLaunchKernelGGL(k, dim3((uint32_t)nb), dim3(kThreads), 0, stream, x.data_ptr<float>(),
                     reinterpret_cast<bf16_t*>(out.data_ptr()), n, (unsigned long long)seed,
                     (unsigned long long)ordinal, (uint32_t)step, offset);
  XDDP_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------
// Layer-wise trust-ratio optimizers: LAMB and LARS. Both need the L2 norm of whole tensors before
// any element of them is updated, so a step is three stream-ordered launches (per segment table):
//   1. a pass that writes two sums of squares per 8192-element chunk, at the chunk's index in the
//      whole list. A tensor is never split across segment tables, but a list of more than 40
//      tensors is, so partials and ratios are indexed over the list, not over one launch;
//   2. trust_ratio_kernel: one wave per tensor folds that tensor's chunk partials in a fixed order
//      and writes its ratio;
//   3. the update, which reads the ratio through a pointer slot of the segment table.
// A chunk partial depends on its own 8192 elements only and the fold on one tensor's partials only,
// so a tensor's result is bitwise the same alone, in any list, and on every replica.
// ------------------------------------------------------------------------------------
struct TrustArgs {
  bool lars;   // false: LAMB, ratio = |w| / |u|; true: LARS, ratio = tc |w| / (|g'| + wd |w| + eps)
  bool adapt;  // LAMB: false gives ratio 1
  float tc, wd, eps;
  const float* gs;  // LARS: |g'| = |*gs| |g|
};

// Slots {this tensor's chunk partials (pairs of floats), the address of its ratio}; "numel" is the
// tensor's chunk count (0 for a zero-numel tensor: ratio 1). Block s is tensor s. A norm that is
// exactly zero gives ratio 1; a non-finite one is not masked.
__global__ __launch_bounds__(64) void trust_ratio_kernel(SegTable<2> t, TrustArgs a) {
  const int s = blockIdx.x;
  const float* part = reinterpret_cast<const float*>(t.ptr[0][s]);
  const int64_t n = t.numel[s];
  double s0 = 0.0, s1 = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 64) {
    s0 += (double)part[2 * i];
    s1 += (double)part[2 * i + 1];
  }
  s0 = dev::wave_sum(s0);
  s1 = dev::wave_sum(s1);
  if (threadIdx.x != 0) return;
  const double wn = sqrt(s0);
  double r = 1.0;
  if (a.lars) {
    const double gn = sqrt(s1) * fabs(a.gs ? (double)*a.gs : 1.0);
    if (wn != 0.0 && gn != 0.0) r = (double)a.tc * wn / (gn + (double)a.wd * wn + (double)a.eps);
  } else {
    const double un = sqrt(s1);
    if (a.adapt && wn != 0.0 && un != 0.0) r = wn / un;
  }
  *reinterpret_cast<float*>(t.ptr[1][s]) = (float)r;
}

// Chunk layout of a list: tensor i's partials start at pair index start[i]
struct ChunkMap {
  std::vector<int64_t> start, count;
  int64_t total = 0;
  explicit ChunkMap(const std::vector<at::Tensor>& ts) {
    for (auto& x : ts) {
      start.push_back(total);
      count.push_back((x.numel() + kChunk - 1) / kChunk);
      total += count.back();
    }
  }
};

static void launch_trust_ratio(float* partials, float* ratios, const ChunkMap& cm, const TrustArgs& a,
                               hipStream_t stream) {
  SegTable<2> t;
  t.nseg = 0;
  auto flush = [&]() {
    hipLaunchKernelGGL(trust_ratio_kernel, dim3(t.nseg), dim3(64), 0, stream, t, a);
    XDDP_HIP_CHECK(hipGetLastError());
    t.nseg = 0;
  };
  for (size_t i = 0; i < cm.start.size(); ++i) {
    t.ptr[0][t.nseg] = partials + 2 * cm.start[i];
    t.ptr[1][t.nseg] = ratios + i;
    t.numel[t.nseg] = cm.count[i];
    t.blk_end[t.nseg] = t.nseg + 1;
    if (++t.nseg == kMaxSeg) flush();
  }
  if (t.nseg) flush();
}

// ---- LAMB ---------------------------------------------------------------------------
struct LambArgs {
  float lr, b1, b2, omb1, omb2, eps, wd, bc1, bc2_sqrt;
  bool maximize;
  const float* gs;
};

// The update direction u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd w. Stage 1 takes its norm
// and stage 3 applies it: both call this one function, compiled without contraction (the one FMA
// is explicit), so the norm is exactly the norm of what is applied.
__device__ __forceinline__ float lamb_dir(const LambArgs& a, float w, float m, float v) {
#pragma clang fp contract(off)
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  const float q = (m / a.bc1) / denom;
  return a.wd != 0.f ? fmaf(a.wd, w, q) : q;
}

// Stage 1, slots {w (the fp32 master, or the parameter), grad, exp_avg, exp_avg_sq, this tensor's
// chunk partials}: updates the moments, forms u in registers and writes sum(w^2), sum(u^2) of the chunk.
struct LambMoments {
  const LambArgs& a;
  const float gscale;
  float sw = 0.f, su = 0.f;
  __device__ __forceinline__ explicit LambMoments(const LambArgs& a_)
      : a(a_), gscale((a_.gs ? *a_.gs : 1.f) * (a_.maximize ? -1.f : 1.f)) {}
  __device__ __forceinline__ void operator()(float wv, float gv, float& mv, float& vv) {
    const float gg = gv * gscale;
    mv = fmaf(a.b1, mv, a.omb1 * gg);
    vv = fmaf(a.b2, vv, a.omb2 * gg * gg);
    const float u = lamb_dir(a, wv, mv, vv);
    sw = fmaf(wv, wv, sw);
    su = fmaf(u, u, su);
  }
};

template <typename W, typename G, bool VEC>
__global__ __launch_bounds__(kThreads) void lamb_moments_kernel(SegTable<5> t, LambArgs a) {
  __shared__ float scratch[kThreads / 64];
  const Chunk c = block_chunk(t);
  const W* w = reinterpret_cast<const W*>(t.ptr[0][c.s]);
  const G* g = reinterpret_cast<const G*>(t.ptr[1][c.s]);
  float* m = reinterpret_cast<float*>(t.ptr[2][c.s]);
  float* v = reinterpret_cast<float*>(t.ptr[3][c.s]);
  float* part = reinterpret_cast<float*>(t.ptr[4][c.s]) + 2 * (c.base / kChunk);
  const int64_t n = c.n;
  LambMoments upd(a);
  if (VEC && c.base + kChunk <= n) {  // whole chunk: every load first (see adam_kernel)
    float wv[kIters][8], gv[kIters][8], mv[kIters][8], vv[kIters][8];
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int64_t i = c.base + ((int64_t)it * kThreads + threadIdx.x) * 8;
      Vec8<W>::ld(w + i, wv[it]);
      Vec8<G>::ld(g + i, gv[it]);
      Vec8<float>::ld(m + i, mv[it]);
      Vec8<float>::ld(v + i, vv[it]);
    }
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int64_t i = c.base + ((int64_t)it * kThreads + threadIdx.x) * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) upd(wv[it][j], gv[it][j], mv[it][j], vv[it][j]);
      Vec8<float>::st(m + i, mv[it]);
      Vec8<float>::st(v + i, vv[it]);
    }
  } else {
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int64_t i = c.base + ((int64_t)it * kThreads + threadIdx.x) * 8;
      if (VEC && i + 8 <= n) {
        float wv[8], gv[8], mv[8], vv[8];
        Vec8<W>::ld(w + i, wv);
        Vec8<G>::ld(g + i, gv);
        Vec8<float>::ld(m + i, mv);
        Vec8<float>::ld(v + i, vv);
#pragma unroll
        for (int j = 0; j < 8; ++j) upd(wv[j], gv[j], mv[j], vv[j]);
        Vec8<float>::st(m + i, mv);
        Vec8<float>::st(v + i, vv);
      } else {
        for (int64_t k = i; k < i + 8 && k < n; ++k) {
          float mv = m[k], vv = v[k];
          upd(Elem<W, float>::ld(w, k), Elem<G, float>::ld(g, k), mv, vv);
          m[k] = mv;
          v[k] = vv;
        }
      }
    }
  }
  const float sw = dev::block_sum(upd.sw, scratch);
  const float su = dev::block_sum(upd.su, scratch);
  if (threadIdx.x == 0) {
    part[0] = sw;
    part[1] = su;
  }
}

// Stage 3, slots {w (the fp32 master, or the parameter), exp_avg, exp_avg_sq, the address of the
// tensor's ratio, the model's parameter (MASTER)}: w <- w - lr r u, u recomputed from the stored moments.
template <typename P, bool VEC, bool MASTER>
__global__ __launch_bounds__(kThreads) void lamb_apply_kernel(SegTable<5> t, LambArgs a) {
  using W = std::conditional_t<MASTER, float, P>;
  const Chunk c = block_chunk(t);
  W* w = reinterpret_cast<W*>(t.ptr[0][c.s]);
  const float* m = reinterpret_cast<const float*>(t.ptr[1][c.s]);
  const float* v = reinterpret_cast<const float*>(t.ptr[2][c.s]);
  const float step = -a.lr * *reinterpret_cast<const float*>(t.ptr[3][c.s]);
  P* q = nullptr;
  if constexpr (MASTER) q = reinterpret_cast<P*>(t.ptr[4][c.s]);
  const int64_t n = c.n;
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int64_t i = c.base + ((int64_t)it * kThreads + threadIdx.x) * 8;
    if (VEC && i + 8 <= n) {
      float wv[8], mv[8], vv[8];
      Vec8<W>::ld(w + i, wv);
      Vec8<float>::ld(m + i, mv);
      Vec8<float>::ld(v + i, vv);
#pragma unroll
      for (int j = 0; j < 8; ++j) wv[j] = fmaf(step, lamb_dir(a, wv[j], mv[j], vv[j]), wv[j]);
      Vec8<W>::st(w + i, wv);
      if (MASTER) Vec8<P>::st(q + i, wv);
    } else {
      for (int64_t k = i; k < i + 8 && k < n; ++k) {
        float wv = Elem<W, float>::ld(w, k);
        wv = fmaf(step, lamb_dir(a, wv, m[k], v[k]), wv);
        Elem<W, float>::st(w, k, wv);
        if (MASTER) Elem<P, float>::st(q, k, wv);
      }
    }
  }
}

at::Tensor fused_lamb(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                      const std::vector<at::Tensor>& exp_avgs, const std::vector<at::Tensor>& exp_avg_sqs,
                      const std::vector<at::Tensor>& masters, double lr, double beta1, double beta2, double eps,
                      double weight_decay, int64_t step, bool bias_correction, bool adapt, bool maximize,
                      const c10::optional<at::Tensor>& grad_scale, hipStream_t stream) {
  const size_t N = params.size();
  TORCH_CHECK(N > 0, "lamb: empty tensor list");
  TORCH_CHECK(grads.size() == N && exp_avgs.size() == N && exp_avg_sqs.size() == N, "lamb: list length mismatch");
  const bool has_master = !masters.empty();
  TORCH_CHECK(!has_master || masters.size() == N, "lamb: masters length mismatch");
  TORCH_CHECK(step >= 1, "lamb: step must be >= 1");
  const auto pt = params[0].scalar_type(), gt = grads[0].scalar_type();
  TORCH_CHECK(pt != at::kDouble && gt != at::kDouble, "fused LAMB: fp64 unsupported");
  TORCH_CHECK(!has_master || pt == at::kBFloat16 || pt == at::kHalf, "master-weight LAMB: model params must be bf16/fp16");
  check_adam_lists("lamb", params, grads, {&exp_avgs, &exp_avg_sqs}, masters, nullptr, nullptr);
  const ChunkMap cm(params);
  const auto f32 = at::TensorOptions().dtype(at::kFloat).device(params[0].device());
  at::Tensor partials = at::empty({2 * std::max<int64_t>(cm.total, 1)}, f32);
  at::Tensor ratios = at::empty({(int64_t)N}, f32);
  float* part = partials.data_ptr<float>();
  float* rat = ratios.data_ptr<float>();
  std::vector<std::array<void*, 5>> p1, p3;
  std::vector<int64_t> numels;
  bool vec1 = true, vec3 = true;
  for (size_t i = 0; i < N; ++i) {
    void* w = has_master ? masters[i].data_ptr() : params[i].data_ptr();
    p1.push_back({w, const_cast<void*>(grads[i].data_ptr()), exp_avgs[i].data_ptr(), exp_avg_sqs[i].data_ptr(),
                  part + 2 * cm.start[i]});
    p3.push_back({w, exp_avgs[i].data_ptr(), exp_avg_sqs[i].data_ptr(), rat + i,
                  has_master ? params[i].data_ptr() : nullptr});
    numels.push_back(params[i].numel());
    for (int q = 0; q < 4; ++q) vec1 = vec1 && aligned16(p1.back()[q]);
    vec3 = vec3 && aligned16(w) && aligned16(p3.back()[1]) && aligned16(p3.back()[2]) && aligned16(p3.back()[4]);
  }
  const double bc1 = bias_correction ? 1.0 - std::pow(beta1, (double)step) : 1.0;
  const double bc2 = bias_correction ? 1.0 - std::pow(beta2, (double)step) : 1.0;
  const LambArgs args = {(float)lr,  (float)beta1,        (float)beta2, (float)(1.0 - beta1),  (float)(1.0 - beta2),
                         (float)eps, (float)weight_decay, (float)bc1,   (float)std::sqrt(bc2), maximize,
                         scale_ptr(grad_scale)};
  const auto wt = has_master ? at::kFloat : pt;
  XDDP_DISPATCH_FLOAT_NO_F64(wt, W, "fused LAMB: unsupported parameter dtype ",
    XDDP_DISPATCH_FLOAT_NO_F64(gt, G, "fused LAMB: unsupported gradient dtype ", {
      launch_list<5>(vec1 ? lamb_moments_kernel<W, G, true> : lamb_moments_kernel<W, G, false>, p1, numels, args, stream);
    }));
  launch_trust_ratio(part, rat, cm, TrustArgs{false, adapt, 0.f, 0.f, 0.f, nullptr}, stream);
  XDDP_DISPATCH_FLOAT_NO_F64(pt, P, "fused LAMB: unsupported parameter dtype ", {
    if (has_master) {
      if constexpr (!std::is_same<P, float>::value)
        launch_list<5>(vec3 ? lamb_apply_kernel<P, true, true> : lamb_apply_kernel<P, false, true>, p3, numels, args, stream);
    } else {
      launch_list<5>(vec3 ? lamb_apply_kernel<P, true, false> : lamb_apply_kernel<P, false, false>, p3, numels, args, stream);
    }
  });
  return ratios;
}

// ---- LARS ---------------------------------------------------------------------------
// Slots {w, grad, this tensor's chunk partials}: sum(w^2), sum(g^2) of the chunk (g unscaled:
// the finalize multiplies its norm by |grad_scale| once).
template <typename W, typename G, bool VEC>
__global__ __launch_bounds__(kThreads) void sumsq2_kernel(SegTable<3> t) {
  __shared__ float scratch[kThreads / 64];
  const Chunk c = block_chunk(t);
  const W* w = reinterpret_cast<const W*>(t.ptr[0][c.s]);
  const G* g = reinterpret_cast<const G*>(t.ptr[1][c.s]);
  float* part = reinterpret_cast<float*>(t.ptr[2][c.s]) + 2 * (c.base / kChunk);
  const int64_t n = c.n;
  float sw = 0.f, sg = 0.f;
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int64_t i = c.base + ((int64_t)it * kThreads + threadIdx.x) * 8;
    if (VEC && i + 8 <= n) {
      float wv[8], gv[8];
      Vec8<W>::ld(w + i, wv);
      Vec8<G>::ld(g + i, gv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sw = fmaf(wv[j], wv[j], sw);
        sg = fmaf(gv[j], gv[j], sg);
      }
    } else {
      for (int64_t k = i; k < i + 8 && k < n; ++k) {
        const float wv = Elem<W, float>::ld(w, k), gv = Elem<G, float>::ld(g, k);
        sw = fmaf(wv, wv, sw);
        sg = fmaf(gv, gv, sg);
      }
    }
  }
  sw = dev::block_sum(sw, scratch);
  sg = dev::block_sum(sg, scratch);
  if (threadIdx.x == 0) {
    part[0] = sw;
    part[1] = sg;
  }
}

at::Tensor fused_lars(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                      const std::vector<at::Tensor>& momentum_bufs, const std::vector<at::Tensor>& masters, double lr,
                      double momentum, double dampening, double weight_decay, bool nesterov, bool maximize,
                      bool first_step, double trust_coefficient, double eps,
                      const c10::optional<at::Tensor>& grad_scale, hipStream_t stream) {
  const size_t N = params.size();
  TORCH_CHECK(N > 0, "lars: empty tensor list");
  TORCH_CHECK(grads.size() == N, "lars: list length mismatch");
  const bool mom = momentum != 0.0, has_master = !masters.empty();
  TORCH_CHECK(!mom || momentum_bufs.size() == N, "lars: momentum buffers missing");
  TORCH_CHECK(!has_master || masters.size() == N, "lars: masters length mismatch");
  const auto pt = params[0].scalar_type(), gt = grads[0].scalar_type();
  TORCH_CHECK(pt != at::kDouble && gt != at::kDouble, "fused LARS: fp64 unsupported");
  TORCH_CHECK(!has_master || pt == at::kBFloat16 || pt == at::kHalf, "master-weight LARS: model params must be bf16/fp16");
  if (mom) check_adam_lists("lars", params, grads, {&momentum_bufs}, masters, nullptr, nullptr);
  else check_adam_lists("lars", params, grads, {}, masters, nullptr, nullptr);
  const ChunkMap cm(params);
  const auto f32 = at::TensorOptions().dtype(at::kFloat).device(params[0].device());
  at::Tensor partials = at::empty({2 * std::max<int64_t>(cm.total, 1)}, f32);
  at::Tensor ratios = at::empty({(int64_t)N}, f32);
  float* part = partials.data_ptr<float>();
  float* rat = ratios.data_ptr<float>();
  std::vector<std::array<void*, 3>> p1;
  std::vector<std::array<void*, 4>> p3;   // {param, grad, buf, ratio}
  std::vector<std::array<void*, 5>> p3m;  // {master, grad, buf, param, ratio}
  std::vector<int64_t> numels;
  bool vec1 = true, vec3 = true;
  for (size_t i = 0; i < N; ++i) {
    void* w = has_master ? masters[i].data_ptr() : params[i].data_ptr();
    void* g = const_cast<void*>(grads[i].data_ptr());
    void* b = mom ? momentum_bufs[i].data_ptr() : nullptr;
    p1.push_back({w, g, part + 2 * cm.start[i]});
    if (has_master) p3m.push_back({w, g, b, params[i].data_ptr(), rat + i});
    else p3.push_back({w, g, b, rat + i});
    numels.push_back(params[i].numel());
    vec1 = vec1 && aligned16(w) && aligned16(g);
    vec3 = vec3 && aligned16(w) && aligned16(g) && aligned16(b) && aligned16(params[i].data_ptr());
  }
  const SgdArgs args = sgd_args(lr, momentum, dampening, weight_decay, nesterov, maximize, first_step, grad_scale);
  const auto wt = has_master ? at::kFloat : pt;
  XDDP_DISPATCH_FLOAT_NO_F64(wt, W, "fused LARS: unsupported parameter dtype ",
    XDDP_DISPATCH_FLOAT_NO_F64(gt, G, "fused LARS: unsupported gradient dtype ", {
      auto k = vec1 ? sumsq2_kernel<W, G, true> : sumsq2_kernel<W, G, false>;
      for_each_table<3>(p1, numels, [&](const SegTable<3>& t, int32_t nb) {
        hipLaunchKernelGGL(k, dim3(nb), dim3(kThreads), 0, stream, t);
        XDDP_HIP_CHECK(hipGetLastError());
      });
    }));
  launch_trust_ratio(part, rat, cm,
                     TrustArgs{true, true, (float)trust_coefficient, (float)weight_decay, (float)eps,
                               scale_ptr(grad_scale)},
                     stream);
  XDDP_DISPATCH_FLOAT_NO_F64(pt, P, "fused LARS: unsupported parameter dtype ",
    XDDP_DISPATCH_FLOAT_NO_F64(gt, G, "fused LARS: unsupported gradient dtype ", {
      if (has_master) {
        if constexpr (!std::is_same<P, float>::value)
          launch_list<5>(vec3 ? (mom ? sgd_kernel<P, G, true, true, true, true> : sgd_kernel<P, G, true, false, true, true>)
                              : (mom ? sgd_kernel<P, G, false, true, true, true> : sgd_kernel<P, G, false, false, true, true>),
                         p3m, numels, args, stream);
      } else {
        launch_list<4>(vec3 ? (mom ? sgd_kernel<P, G, true, true, false, true> : sgd_kernel<P, G, true, false, false, true>)
                            : (mom ? sgd_kernel<P, G, false, true, false, true> : sgd_kernel<P, G, false, false, false, true>),
                       p3, numels, args, stream);
      }
    }));
  return ratios;
}

}  // namespace kernels
}  // namespace xddp

