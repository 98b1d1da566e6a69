// Softmax cross-entropy for every head (cross_entropy.hip serves only the bf16 LM head with a class
// count divisible by 8 and default arguments): fp32 / bf16 / fp16 logits [R, C], any C >= 1 and
// any row alignment, label smoothing eps, z-loss z, and the reductions none / sum / mean.
//
//   row loss      keep · [ (1 - eps)(lse - x_t) + eps (lse - mean_c x) + z lse² ]
//   row gradient  g_r · keep · [ p (1 + 2 z lse) - (1 - eps) onehot_t - eps / C ],   p = exp(x - lse)
//
// with keep = target != ignore_index and g_r the upstream gradient (per row for "none", g for
// "sum", g / count for "mean"; count = kept rows, at least 1). Ignored rows give 0 and a zero
// gradient; a target outside [0, C) that is not ignore_index gives NaN, a zero gradient and sets
// the device flag, as cross_entropy.hip does. fp32 math throughout.
//
// Narrow rows (C <= 1024, the classification heads: [32, 10] fp32, [256, 1000] bf16): one wave per
// row, four rows per 256-thread block, lane-strided (coalesced) scalar loads, the row held in
// registers (up to 16 values per lane, the trip count a template argument), so the forward reads
// the logits once; max, sum-exp, sum x and x_t come from shuffles alone: no LDS and no barrier.
// Wide rows (C > 1024): one block per row and the online (max, sum) scheme of cross_entropy.hip
// with its -inf handling, over a 16-B aligned body between a scalar head and tail, so a row may
// start at any element (C · esize % 16 != 0 misaligns every row differently).
// Finalize: one block sums the row losses and counts the kept rows in a fixed order and leaves the
// reduced loss and the count on the device, where the backward reads the count. A "mean" forward
// is two launches, a backward one, and every result is bitwise repeatable.
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <cmath>

#include "common.h"
#include "kernels/dev_utils.h"

namespace xddp {
namespace kernels {

namespace {

constexpr int kRT = 256;           // threads per block
constexpr int kRowsPerBlock = 4;   // narrow kernels: one wave per row
constexpr int kNarrowMax = 1024;   // 16 trips x 64 lanes

// fp32 logits are checked against fp32 rounding alone (no storage ulp to hide in): the exact expf
template <typename T>
__device__ __forceinline__ float ex(float a) {
  if constexpr (__is_same(T, float)) return expf(a);
  else return __expf(a);
}

template <typename T>
__device__ __forceinline__ void merge(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  if (M == -INFINITY) return;  // both empty
  s = s * ex<T>(m - M) + s2 * ex<T>(m2 - M);
  m = M;
}

// eps = 0 and z = 0 leave out their terms (0 · inf with a masked logit, and exactly lse - x_t)
__device__ __forceinline__ float row_loss(float lse, float xt, float sx, int C, int64_t t, int64_t ignore_index,
                                          float eps, float z, int* bad) {
  if (t == ignore_index) return 0.f;
  if (t < 0 || t >= C) {
    atomicOr(bad, 1);
    return NAN;
  }
  float l = (1.f - eps) * (lse - xt);
  if (eps > 0.f) l += eps * (lse - sx / (float)C);
  if (z > 0.f) l += z * lse * lse;
  return l;
}

struct GradCoef {
  float a, b, e, gs;  // d = (p · a - onehot · b - e) · gs
  bool skip;
};
__device__ __forceinline__ GradCoef grad_coef(int64_t r, int64_t t, int C, int64_t ignore_index, float lse, float eps,
                                              float z, const float* g, int g_per_row, const float* count) {
  GradCoef k;
  k.skip = t == ignore_index || t < 0 || t >= C;
  k.gs = k.skip ? 0.f : g[g_per_row ? r : 0];
  if (count != nullptr) k.gs /= count[0];
  k.a = z > 0.f ? 1.f + 2.f * z * lse : 1.f;
  k.b = 1.f - eps;
  k.e = eps / (float)C;
  return k;
}
template <typename T>
__device__ __forceinline__ float grad_elem(const GradCoef& k, float x, float lse, bool is_target) {
  return k.skip ? 0.f : (ex<T>(x - lse) * k.a - (is_target ? k.b : 0.f) - k.e) * k.gs;
}

// ---- narrow rows: one wave per row, the row in registers ------------------------------------
template <typename T, int TRIPS>
__global__ __launch_bounds__(kRT) void xent_narrow_fwd_kernel(const T* __restrict__ logits,
                                                              const int64_t* __restrict__ target,
                                                              float* __restrict__ loss, float* __restrict__ lse,
                                                              int* __restrict__ bad, int64_t R, int C,
                                                              int64_t ignore_index, float eps, float z) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= R) return;  // a whole wave leaves; there is no barrier below
  const T* row = logits + r * C;
  const int64_t t = target[r];
  float v[TRIPS];
  float m = -INFINITY, sx = 0.f, xt = 0.f;
#pragma unroll
  for (int k = 0; k < TRIPS; ++k) {
    const int c = k * 64 + lane;
    v[k] = -INFINITY;
    if (c < C) {
      v[k] = dev::Elem<T, float>::ld(row, c);
      sx += v[k];
      if (c == t) xt = v[k];
    }
    m = fmaxf(m, v[k]);
  }
  m = dev::wave_max(m);
  const float Ms = m == -INFINITY ? 0.f : m;  // a row of -inf: exp(-inf - 0) = 0, not exp(-inf + inf)
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < TRIPS; ++k) s += ex<T>(v[k] - Ms);  // padding: exp(-inf) = 0
  s = dev::wave_sum(s);
  sx = dev::wave_sum(sx);
  xt = dev::wave_sum(xt);  // one lane holds x_t, the others 0
  if (lane == 0) {
    const float l = m + logf(s);
    lse[r] = l;
    loss[r] = row_loss(l, xt, sx, C, t, ignore_index, eps, z, bad);
  }
}

template <typename T, int TRIPS>
__global__ __launch_bounds__(kRT) void xent_narrow_bwd_kernel(const T* __restrict__ logits,
                                                              const int64_t* __restrict__ target,
                                                              const float* __restrict__ lse,
                                                              const float* __restrict__ g,
                                                              const float* __restrict__ count,
                                                              T* __restrict__ dlogits, int64_t R, int C,
                                                              int64_t ignore_index, float eps, float z,
                                                              int g_per_row) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= R) return;
  const T* row = logits + r * C;
  T* drow = dlogits + r * C;
  const int64_t t = target[r];
  const float l = lse[r];
  const GradCoef k = grad_coef(r, t, C, ignore_index, l, eps, z, g, g_per_row, count);
  float x[TRIPS];
#pragma unroll
  for (int i = 0; i < TRIPS; ++i) {
    const int c = i * 64 + lane;
    x[i] = c < C ? dev::Elem<T, float>::ld(row, c) : 0.f;
  }
#pragma unroll
  for (int i = 0; i < TRIPS; ++i) {
    const int c = i * 64 + lane;
    if (c < C) dev::Elem<T, float>::st(drow, c, grad_elem<T>(k, x[i], l, c == t));
  }
}

// ---- wide rows: one block per row, scalar head and tail around an aligned 16-B body ---------
// Elements in front of the first 16-B boundary of a row (0 .. 7 for 2-byte types, 0 .. 3 for fp32).
template <typename T>
__device__ __forceinline__ int row_head(const T* row, int C) {
  const int h = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) / sizeof(T));
  return h < C ? h : C;
}

template <typename T, bool SMOOTH>
__global__ __launch_bounds__(kRT) void xent_wide_fwd_kernel(const T* __restrict__ logits,
                                                            const int64_t* __restrict__ target,
                                                            float* __restrict__ loss, float* __restrict__ lse,
                                                            int* __restrict__ bad, int C, int64_t ignore_index,
                                                            float eps, float z) {
  const int64_t r = blockIdx.x;
  const T* row = logits + r * C;
  const int head = row_head(row, C);
  const int nvec = (C - head) / 8, tail0 = head + nvec * 8, ntail = C - tail0;  // head, ntail < 8
  float m = -INFINITY, s = 0.f, sx = 0.f;
  if (threadIdx.x < 16) {  // threads 0 .. 7: head element j; threads 8 .. 15: tail element j
    const int j = threadIdx.x & 7;
    const bool is_tail = threadIdx.x >= 8;
    if (j < (is_tail ? ntail : head)) {
      const float x = dev::Elem<T, float>::ld(row, is_tail ? tail0 + j : j);
      m = x;
      s = x == -INFINITY ? 0.f : 1.f;  // exp(x - x), or nothing finite yet
      sx = x;
    }
  }
  const T* body = row + head;
  for (int i = threadIdx.x; i < nvec; i += kRT) {
    float v[8];
    dev::Vec8<T>::ld(body + (int64_t)i * 8, v);
    float vm = v[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) vm = fmaxf(vm, v[j]);
    const float M = fmaxf(m, vm);
    // nothing finite yet (a chunk of -inf, or a first chunk of -inf): subtract 0, so every term is
    // exp(-inf) = 0 and not exp(-inf + inf) = NaN
    const float Ms = M == -INFINITY ? 0.f : M;
    float acc = s * ex<T>(m - Ms);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += ex<T>(v[j] - Ms);
    if (SMOOTH) {
#pragma unroll
      for (int j = 0; j < 8; ++j) sx += v[j];
    }
    m = M;
    s = acc;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) merge<T>(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
  sx = dev::wave_sum(sx);
  __shared__ float sm[kRT / 64], ss[kRT / 64], sxs[kRT / 64];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    sm[wid] = m;
    ss[wid] = s;
    sxs[wid] = sx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = sm[0], S = ss[0], SX = sxs[0];
    for (int w = 1; w < kRT / 64; ++w) {
      merge<T>(M, S, sm[w], ss[w]);
      SX += sxs[w];
    }
    const float l = M + logf(S);
    lse[r] = l;
    const int64_t t = target[r];
    const float xt = t >= 0 && t < C ? dev::Elem<T, float>::ld(row, t) : 0.f;
    loss[r] = row_loss(l, xt, SX, C, t, ignore_index, eps, z, bad);
  }
}

template <typename T>
__global__ __launch_bounds__(kRT) void xent_wide_bwd_kernel(const T* __restrict__ logits,
                                                            const int64_t* __restrict__ target,
                                                            const float* __restrict__ lse, const float* __restrict__ g,
                                                            const float* __restrict__ count, T* __restrict__ dlogits,
                                                            int C, int64_t ignore_index, float eps, float z,
                                                            int g_per_row) {
  const int64_t r = blockIdx.x;
  const T* row = logits + r * C;
  T* drow = dlogits + r * C;  // same misalignment as row: both bases are 16-B aligned
  const int head = row_head(row, C);
  const int nvec = (C - head) / 8, tail0 = head + nvec * 8, ntail = C - tail0;
  const int64_t t = target[r];
  const float l = lse[r];
  const GradCoef k = grad_coef(r, t, C, ignore_index, l, eps, z, g, g_per_row, count);
  if (threadIdx.x < 16) {
    const int j = threadIdx.x & 7;
    const bool is_tail = threadIdx.x >= 8;
    if (j < (is_tail ? ntail : head)) {
      const int c = is_tail ? tail0 + j : j;
      dev::Elem<T, float>::st(drow, c, grad_elem<T>(k, dev::Elem<T, float>::ld(row, c), l, c == t));
    }
  }
  for (int i = threadIdx.x; i < nvec; i += kRT) {
    const int c0 = head + i * 8;
    float v[8], d[8];
    dev::Vec8<T>::ld(row + c0, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = grad_elem<T>(k, v[j], l, c0 + j == t);
    dev::st8_stream(drow + c0, d);
  }
}

// ---- finalize: the reduced loss and the kept-row count, one block, fixed order ---------------
__global__ __launch_bounds__(kRT) void xent_finalize_kernel(const float* __restrict__ loss,
                                                            const int64_t* __restrict__ target,
                                                            float* __restrict__ reduced, float* __restrict__ count,
                                                            int64_t R, int64_t ignore_index, int mean) {
  double a = 0.0;
  int n = 0;
  for (int64_t r = threadIdx.x; r < R; r += kRT) {
    a += (double)loss[r];
    n += target[r] != ignore_index ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    n += __shfl_xor(n, o, 64);
  }
  __shared__ double sa[kRT / 64];
  __shared__ int sn[kRT / 64];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    sa[wid] = a;
    sn[wid] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double A = sa[0];
    int N = sn[0];
    for (int w = 1; w < kRT / 64; ++w) {
      A += sa[w];
      N += sn[w];
    }
    N = N < 1 ? 1 : N;  // every row ignored: a finite 0
    count[0] = (float)N;
    reduced[0] = (float)(mean ? A / (double)N : A);
  }
}

// ---- host side --------------------------------------------------------------------------------
void check_rows(const at::Tensor& logits, const at::Tensor& target) {
  const auto st = logits.scalar_type();
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.is_contiguous() &&
                  (st == at::kFloat || st == at::kBFloat16 || st == at::kHalf),
              "cross_entropy_rows: logits must be a contiguous 2-D fp32 / bf16 / fp16 CUDA tensor");
  TORCH_CHECK(target.is_cuda() && target.scalar_type() == at::kLong && target.dim() == 1 &&
                  target.size(0) == logits.size(0) && target.is_contiguous() && target.device() == logits.device(),
              "cross_entropy_rows: target must be int64 [rows] on the logits' device");
  TORCH_CHECK(logits.size(1) >= 1 && logits.size(1) < (int64_t(1) << 31) && logits.size(0) < (int64_t(1) << 31),
              "cross_entropy_rows: need 1 <= classes < 2^31 and rows < 2^31");
  // rows may start anywhere, but the gradient's rows must be misaligned like the logits' rows
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0,
              "cross_entropy_rows: the logits' base address must be 16-B aligned");
}

int narrow_trips(int64_t C) {
  const int64_t need = (C + 63) / 64;
  int t = 1;
  while (t < need) t *= 2;
  return t;
}

template <typename T>
void launch_forward(const at::Tensor& logits, const at::Tensor& target, float* loss, float* lse, int* bad,
                    int64_t ignore_index, float eps, float z, hipStream_t stream) {
  const int64_t R = logits.size(0);
  const int C = (int)logits.size(1);
  const T* x = reinterpret_cast<const T*>(logits.data_ptr());
  const int64_t* t = target.data_ptr<int64_t>();
  if (C <= kNarrowMax) {
    const dim3 grid((unsigned)((R + kRowsPerBlock - 1) / kRowsPerBlock));
#define XDDP_NARROW_FWD(N)                                                                                        \
  case N:                                                                                                         \
    hipLaunchKernelGGL((xent_narrow_fwd_kernel<T, N>), grid, dim3(kRT), 0, stream, x, t, loss, lse, bad, R, C,    \
                       ignore_index, eps, z);                                                                     \
    break;
    switch (narrow_trips(C)) {
      XDDP_NARROW_FWD(1)
      XDDP_NARROW_FWD(2)
      XDDP_NARROW_FWD(4)
      XDDP_NARROW_FWD(8)
      XDDP_NARROW_FWD(16)
    }
#undef XDDP_NARROW_FWD
  } else if (eps > 0.f) {
    hipLaunchKernelGGL((xent_wide_fwd_kernel<T, true>), dim3((unsigned)R), dim3(kRT), 0, stream, x, t, loss, lse, bad,
                       C, ignore_index, eps, z);
  } else {
    hipLaunchKernelGGL((xent_wide_fwd_kernel<T, false>), dim3((unsigned)R), dim3(kRT), 0, stream, x, t, loss, lse, bad,
                       C, ignore_index, eps, z);
  }
}

template <typename T>
void launch_backward(const at::Tensor& logits, const at::Tensor& target, const float* lse, const float* g,
                     const float* count, at::Tensor& d, int64_t ignore_index, float eps, float z, int g_per_row,
                     hipStream_t stream) {
  const int64_t R = logits.size(0);
  const int C = (int)logits.size(1);
  const T* x = reinterpret_cast<const T*>(logits.data_ptr());
  T* dx = reinterpret_cast<T*>(d.data_ptr());
  const int64_t* t = target.data_ptr<int64_t>();
  if (C <= kNarrowMax) {
    const dim3 grid((unsigned)((R + kRowsPerBlock - 1) / kRowsPerBlock));
#define XDDP_NARROW_BWD(N)                                                                                        \
  case N:                                                                                                         \
    hipLaunchKernelGGL((xent_narrow_bwd_kernel<T, N>), grid, dim3(kRT), 0, stream, x, t, lse, g, count, dx, R, C, \
                       ignore_index, eps, z, g_per_row);                                                          \
    break;
    switch (narrow_trips(C)) {
      XDDP_NARROW_BWD(1)
      XDDP_NARROW_BWD(2)
      XDDP_NARROW_BWD(4)
      XDDP_NARROW_BWD(8)
      XDDP_NARROW_BWD(16)
    }
#undef XDDP_NARROW_BWD
  } else {
    hipLaunchKernelGGL((xent_wide_bwd_kernel<T>), dim3((unsigned)R), dim3(kRT), 0, stream, x, t, lse, g, count, dx, C,
                       ignore_index, eps, z, g_per_row);
  }
}

#define XDDP_XENT_DISPATCH(ST, ...)                   \
  if ((ST) == at::kFloat) {                           \
    using T = float;                                  \
    __VA_ARGS__;                                      \
  } else if ((ST) == at::kBFloat16) {                 \
    using T = dev::bf16_t;                            \
    __VA_ARGS__;                                      \
  } else {                                            \
    using T = dev::f16_t;                             \
    __VA_ARGS__;                                      \
  }

}  // namespace

// reduction 0 none | 1 sum | 2 mean -> {loss per row fp32 [R], lse per row fp32 [R]} and, for sum and
// mean, {reduced loss fp32 [], kept-row count (at least 1) fp32 [1]}. Rows with target ==
// ignore_index give 0, rows with a target outside [0, C) give NaN and set bad[0] (int32 on the
// device, never cleared here). No launch when R == 0 (the reduced loss is 0 then).
std::vector<at::Tensor> cross_entropy_rows_forward(const at::Tensor& logits, const at::Tensor& target,
                                                   int64_t ignore_index, double label_smoothing, double z_loss,
                                                   int64_t reduction, const at::Tensor& bad) {
  check_rows(logits, target);
  TORCH_CHECK(bad.is_cuda() && bad.scalar_type() == at::kInt && bad.numel() >= 1 && bad.device() == logits.device(),
              "cross_entropy_rows: bad-target flag must be an int32 tensor on the logits' device");
  TORCH_CHECK(label_smoothing >= 0.0 && label_smoothing < 1.0 && z_loss >= 0.0 && reduction >= 0 && reduction <= 2,
              "cross_entropy_rows: need 0 <= label_smoothing < 1, z_loss >= 0 and reduction in {0, 1, 2}");
  const int64_t R = logits.size(0);
  const auto f32 = logits.options().dtype(at::kFloat);
  auto loss = at::empty({R}, f32);
  auto lse = at::empty({R}, f32);
  if (R == 0) {
    if (reduction == 0) return {loss, lse};
    return {loss, lse, at::zeros({}, f32), at::ones({1}, f32)};
  }
  auto stream = c10::hip::getCurrentHIPStream(logits.device().index()).stream();
  XDDP_XENT_DISPATCH(logits.scalar_type(),
                     launch_forward<T>(logits, target, loss.data_ptr<float>(), lse.data_ptr<float>(),
                                       bad.data_ptr<int>(), ignore_index, (float)label_smoothing, (float)z_loss, stream))
  XDDP_HIP_CHECK(hipGetLastError());
  if (reduction == 0) return {loss, lse};
  auto reduced = at::empty({}, f32);
  auto count = at::empty({1}, f32);
  hipLaunchKernelGGL(xent_finalize_kernel, dim3(1), dim3(kRT), 0, stream, loss.data_ptr<float>(),
                     target.data_ptr<int64_t>(), reduced.data_ptr<float>(), count.data_ptr<float>(), R, ignore_index,
                     reduction == 2 ? 1 : 0);
  XDDP_HIP_CHECK(hipGetLastError());
  return {loss, lse, reduced, count};
}

// dlogits (the logits' dtype); g fp32 [1] (sum, mean) or [R] (none), count fp32 [1] for mean
at::Tensor cross_entropy_rows_backward(const at::Tensor& logits, const at::Tensor& target, const at::Tensor& lse,
                                       const at::Tensor& g, const c10::optional<at::Tensor>& count,
                                       int64_t ignore_index, double label_smoothing, double z_loss) {
  check_rows(logits, target);
  const int64_t R = logits.size(0);
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat && lse.numel() == R && lse.is_contiguous(),
              "cross_entropy_rows_backward: lse must be fp32 [rows] on the device");
  TORCH_CHECK(g.is_cuda() && g.scalar_type() == at::kFloat && g.is_contiguous() && (g.numel() == 1 || g.numel() == R),
              "cross_entropy_rows_backward: g must be fp32 [1] or [rows] on the device");
  TORCH_CHECK(!count.has_value() ||
                  (count->is_cuda() && count->scalar_type() == at::kFloat && count->numel() == 1 && g.numel() == 1),
              "cross_entropy_rows_backward: count must be fp32 [1] on the device, with a single g");
  auto d = at::empty_like(logits);
  if (R == 0) return d;
  auto stream = c10::hip::getCurrentHIPStream(logits.device().index()).stream();
  const float* cnt = count.has_value() ? count->data_ptr<float>() : nullptr;
  XDDP_XENT_DISPATCH(logits.scalar_type(),
                     launch_backward<T>(logits, target, lse.data_ptr<float>(), g.data_ptr<float>(), cnt, d,
                                        ignore_index, (float)label_smoothing, (float)z_loss, g.numel() != 1 ? 1 : 0,
                                        stream))
  XDDP_HIP_CHECK(hipGetLastError());
  return d;
}

}  // namespace kernels
}  // namespace xddp
