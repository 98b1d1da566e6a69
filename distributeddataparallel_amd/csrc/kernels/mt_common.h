// What the multi-tensor HIP files share (multi_tensor.hip, adafactor.hip): the by-value segment
// table of a list launch, its block-to-chunk lookup, the table builder and the dtype dispatch.
#pragma once

#include <ATen/ATen.h>
#include <c10/util/Optional.h>
#include <hip/hip_runtime.h>

#include <array>
#include <vector>

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

static const float* scale_ptr(const c10::optional<at::Tensor>& st) {
  if (!st.has_value() || !st->defined()) return nullptr;
  TORCH_CHECK(st->scalar_type() == at::kFloat && st->is_cuda(), "scale tensor must be a float32 device tensor");
  return st->data_ptr<float>();
}

// Launches `kernel(table, args)` over the list, one launch per segment table.
template <int NPTR, typename K, typename A>
static void launch_list(K kernel, const std::vector<std::array<void*, NPTR>>& ptrs, const std::vector<int64_t>& numels,
                        const A& args, hipStream_t stream) {
  for_each_table<NPTR>(ptrs, numels, [&](const SegTable<NPTR>& t, int32_t nb) {
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(kThreads), 0, stream, t, args);
    XDDP_HIP_CHECK(hipGetLastError());
  });
}

}  // namespace kernels
}  // namespace xddp
