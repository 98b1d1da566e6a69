// Softmax cross-entropy against a two-label target (Mixup / CutMix): the kernels of
// cross_entropy_rows.hip with targets a and b [R] and a device-side weight lam (fp32, 1 or R
// elements), w_a = lam, w_b = 1 - lam, keep = a != ignore_index and b != ignore_index:
//
//   row loss      keep · [ (1 - eps)(lse - w_a x_a - w_b x_b) + eps (lse - mean_c x) + z lse² ]
//   row gradient  g_r · keep · [ p (1 + 2 z lse) - (1 - eps)(w_a onehot_a + w_b onehot_b) - eps / C ]
//
// One read of the logits forward and one read + one write backward, where the composition
// lam CE(x, a) + (1 - lam) CE(x, b) takes two of each and a sum of two gradients.
//
// A weight of exactly 0 contributes nothing: its logit is not read into the loss (0 · -inf would
// be NaN), so lam = 1 gives the bits of cross_entropy_rows on a, and lam = 0 those on b. The
// kernels below follow cross_entropy_rows.hip statement by statement for that reason (same loads,
// same order of the reductions, same expressions); its helpers are repeated here so that file
// stays as it is. A target outside [0, C) on a kept row, whatever its weight, gives NaN, no
// gradient and sets the flag. lam is read from device memory (a captured launch sees the value
// written before each replay); it is not checked to lie in [0, 1].
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

// The weighted target logit; a zero weight leaves its logit out (and the other weight is then 1).
__device__ __forceinline__ float mix_xt(float wa, float wb, float xa, float xb) {
  if (wb == 0.f) return xa;
  if (wa == 0.f) return xb;
  return wa * xa + wb * xb;
}

__device__ __forceinline__ bool in_range(int64_t t, int C) { return t >= 0 && t < C; }

__device__ __forceinline__ float row_loss(float lse, float xt, float sx, int C, int64_t a, int64_t b,
                                          int64_t ignore_index, float eps, float z, int* bad) {
  if (a == ignore_index || b == ignore_index) return 0.f;
  if (!in_range(a, C) || !in_range(b, C)) {
    atomicOr(bad, 1);
    return NAN;
  }
  float l = (1.f - eps) * (lse - xt);
  if (eps > 0.f) l += eps * (lse - sx / (float)C);
  if (z > 0.f) l += z * lse * lse;
  return l;
}

struct GradCoef {
  float a, ba, bb, e, gs;  // d = (p · a - onehot_a · ba - onehot_b · bb - e) · gs
  bool skip;
};
__device__ __forceinline__ GradCoef grad_coef(int64_t r, int64_t ta, int64_t tb, float wa, int C, int64_t ignore_index,
                                              float lse, float eps, float z, const float* g, int g_per_row,
                                              const float* count) {
  GradCoef k;
  k.skip = ta == ignore_index || tb == ignore_index || !in_range(ta, C) || !in_range(tb, C);
  k.gs = k.skip ? 0.f : g[g_per_row ? r : 0];
  if (count != nullptr) k.gs /= count[0];
  k.a = z > 0.f ? 1.f + 2.f * z * lse : 1.f;
  const float b = 1.f - eps;
  k.ba = wa * b;          // lam = 1: b itself
  k.bb = (1.f - wa) * b;  // lam = 0: b itself
  k.e = eps / (float)C;
  return k;
}
// lam in {0, 1}: the subtracted term is b or 0.f, as in the hard-target kernel (b + 0.f = b)
template <typename T>
__device__ __forceinline__ float grad_elem(const GradCoef& k, float x, float lse, bool is_a, bool is_b) {
  const float hot = (is_a ? k.ba : 0.f) + (is_b ? k.bb : 0.f);
  return k.skip ? 0.f : (ex<T>(x - lse) * k.a - hot - k.e) * k.gs;
}

// ---- narrow rows: one wave per row, the row in registers ------------------------------------
template <typename T, int TRIPS>
__global__ __launch_bounds__(kRT) void xent_mixed_narrow_fwd_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ ta, const int64_t* __restrict__ tb,
    const float* __restrict__ lam, int lam_per_row, float* __restrict__ loss, float* __restrict__ lse,
    int* __restrict__ bad, int64_t R, int C, int64_t ignore_index, float eps, float z) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= R) return;  // a whole wave leaves; there is no barrier below
  const T* row = logits + r * C;
  const int64_t a = ta[r], b = tb[r];
  float v[TRIPS];
  float m = -INFINITY, sx = 0.f, xa = 0.f, xb = 0.f;
#pragma unroll
  for (int k = 0; k < TRIPS; ++k) {
    const int c = k * 64 + lane;
    v[k] = -INFINITY;
    if (c < C) {
      v[k] = dev::Elem<T, float>::ld(row, c);
      sx += v[k];
      if (c == a) xa = v[k];
      if (c == b) xb = v[k];
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
  xa = dev::wave_sum(xa);  // one lane holds x_a, the others 0
  xb = dev::wave_sum(xb);
  if (lane == 0) {
    const float l = m + logf(s);
    lse[r] = l;
    const float wa = lam[lam_per_row ? r : 0];
    loss[r] = row_loss(l, mix_xt(wa, 1.f - wa, xa, xb), sx, C, a, b, ignore_index, eps, z, bad);
  }
}

template <typename T, int TRIPS>
__global__ __launch_bounds__(kRT) void xent_mixed_narrow_bwd_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ ta, const int64_t* __restrict__ tb,
    const float* __restrict__ lam, int lam_per_row, const float* __restrict__ lse, const float* __restrict__ g,
    const float* __restrict__ count, T* __restrict__ dlogits, int64_t R, int C, int64_t ignore_index, float eps,
    float z, int g_per_row) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= R) return;
  const T* row = logits + r * C;
  T* drow = dlogits + r * C;
  const int64_t a = ta[r], b = tb[r];
  const float l = lse[r];
  const GradCoef k = grad_coef(r, a, b, lam[lam_per_row ? r : 0], C, ignore_index, l, eps, z, g, g_per_row, count);
  float x[TRIPS];
#pragma unroll
  for (int i = 0; i < TRIPS; ++i) {
    const int c = i * 64 + lane;
    x[i] = c < C ? dev::Elem<T, float>::ld(row, c) : 0.f;
  }
#pragma unroll
  for (int i = 0; i < TRIPS; ++i) {
    const int c = i * 64 + lane;
    if (c < C) dev::Elem<T, float>::st(drow, c, grad_elem<T>(k, x[i], l, c == a, c == b));
  }
}

// ---- wide rows: one block per row, scalar head and tail around an aligned 16-B body ---------
template <typename T>
__device__ __forceinline__ int row_head(const T* row, int C) {
  const int h = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) / sizeof(T));
  return h < C ? h : C;
}

template <typename T, bool SMOOTH>
__global__ __launch_bounds__(kRT) void xent_mixed_wide_fwd_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ ta, const int64_t* __restrict__ tb,
    const float* __restrict__ lam, int lam_per_row, float* __restrict__ loss, float* __restrict__ lse,
    int* __restrict__ bad, int C, int64_t ignore_index, float eps, float z) {
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
    const float Ms = M == -INFINITY ? 0.f : M;  // nothing finite yet: every term is exp(-inf) = 0
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
    const int64_t a = ta[r], b = tb[r];
    const float xa = in_range(a, C) ? dev::Elem<T, float>::ld(row, a) : 0.f;
    const float xb = in_range(b, C) ? dev::Elem<T, float>::ld(row, b) : 0.f;
    const float wa = lam[lam_per_row ? r : 0];
    loss[r] = row_loss(l, mix_xt(wa, 1.f - wa, xa, xb), SX, C, a, b, ignore_index, eps, z, bad);
  }
}

template <typename T>
__global__ __launch_bounds__(kRT) void xent_mixed_wide_bwd_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ ta, const int64_t* __restrict__ tb,
    const float* __restrict__ lam, int lam_per_row, const float* __restrict__ lse, const float* __restrict__ g,
    const float* __restrict__ count, T* __restrict__ dlogits, int C, int64_t ignore_index, float eps, float z,
    int g_per_row) {
  const int64_t r = blockIdx.x;
  const T* row = logits + r * C;
  T* drow = dlogits + r * C;  // same misalignment as row: both bases are 16-B aligned
  const int head = row_head(row, C);
  const int nvec = (C - head) / 8, tail0 = head + nvec * 8, ntail = C - tail0;
  const int64_t a = ta[r], b = tb[r];
  const float l = lse[r];
  const GradCoef k = grad_coef(r, a, b, lam[lam_per_row ? r : 0], C, ignore_index, l, eps, z, g, g_per_row, count);
  if (threadIdx.x < 16) {
    const int j = threadIdx.x & 7;
    const bool is_tail = threadIdx.x >= 8;
    if (j < (is_tail ? ntail : head)) {
      const int c = is_tail ? tail0 + j : j;
      dev::Elem<T, float>::st(drow, c, grad_elem<T>(k, dev::Elem<T, float>::ld(row, c), l, c == a, c == b));
    }
  }
  for (int i = threadIdx.x; i < nvec; i += kRT) {
    const int c0 = head + i * 8;
    float v[8], d[8];
    dev::Vec8<T>::ld(row + c0, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = grad_elem<T>(k, v[j], l, c0 + j == a, c0 + j == b);
    dev::st8_stream(drow + c0, d);
  }
}

// ---- finalize: the reduced loss and the kept-row count, one block, fixed order ---------------
__global__ __launch_bounds__(kRT) void xent_mixed_finalize_kernel(const float* __restrict__ loss,
                                                                  const int64_t* __restrict__ ta,
                                                                  const int64_t* __restrict__ tb,
                                                                  float* __restrict__ reduced,
                                                                  float* __restrict__ count, int64_t R,
                                                                  int64_t ignore_index, int mean) {
  double a = 0.0;
  int n = 0;
  for (int64_t r = threadIdx.x; r < R; r += kRT) {
    a += (double)loss[r];
    n += ta[r] != ignore_index && tb[r] != ignore_index ? 1 : 0;
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
struct Mixed {
  const int64_t* a;
  const int64_t* b;
  const float* lam;
  int lam_per_row;
};

Mixed check_mixed(const at::Tensor& logits, const at::Tensor& a, const at::Tensor& b, const at::Tensor& lam) {
  const auto st = logits.scalar_type();
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.is_contiguous() &&
                  (st == at::kFloat || st == at::kBFloat16 || st == at::kHalf),
              "cross_entropy_mixed: logits must be a contiguous 2-D fp32 / bf16 / fp16 CUDA tensor");
  for (const at::Tensor* t : {&a, &b})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kLong && t->dim() == 1 && t->size(0) == logits.size(0) &&
                    t->is_contiguous() && t->device() == logits.device(),
                "cross_entropy_mixed: targets a and b must be int64 [rows] on the logits' device");
  TORCH_CHECK(lam.is_cuda() && lam.scalar_type() == at::kFloat && lam.is_contiguous() &&
                  lam.device() == logits.device() && (lam.numel() == 1 || lam.numel() == logits.size(0)),
              "cross_entropy_mixed: lam must be fp32 with 1 or [rows] elements on the logits' device");
  TORCH_CHECK(logits.size(1) >= 1 && logits.size(1) < (int64_t(1) << 31) && logits.size(0) < (int64_t(1) << 31),
              "cross_entropy_mixed: need 1 <= classes < 2^31 and rows < 2^31");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0,
              "cross_entropy_mixed: the logits' base address must be 16-B aligned");
  return {a.data_ptr<int64_t>(), b.data_ptr<int64_t>(), lam.data_ptr<float>(), lam.numel() != 1 ? 1 : 0};
}

int narrow_trips(int64_t C) {
  const int64_t need = (C + 63) / 64;
  int t = 1;
  while (t < need) t *= 2;
  return t;
}

template <typename T>
void launch_forward(const at::Tensor& logits, const Mixed& t, float* loss, float* lse, int* bad, int64_t ignore_index,
                    float eps, float z, hipStream_t stream) {
  const int64_t R = logits.size(0);
  const int C = (int)logits.size(1);
  const T* x = reinterpret_cast<const T*>(logits.data_ptr());
  if (C <= kNarrowMax) {
    const dim3 grid((unsigned)((R + kRowsPerBlock - 1) / kRowsPerBlock));
#define XDDP_NARROW_FWD(N)                                                                                     \
  case N:                                                                                                      \
    hipLaunchKernelGGL((xent_mixed_narrow_fwd_kernel<T, N>), grid, dim3(kRT), 0, stream, x, t.a, t.b, t.lam,   \
                       t.lam_per_row, loss, lse, bad, R, C, ignore_index, eps, z);                             \
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
    hipLaunchKernelGGL((xent_mixed_wide_fwd_kernel<T, true>), dim3((unsigned)R), dim3(kRT), 0, stream, x, t.a, t.b,
                       t.lam, t.lam_per_row, loss, lse, bad, C, ignore_index, eps, z);
  } else {
    hipLaunchKernelGGL((xent_mixed_wide_fwd_kernel<T, false>), dim3((unsigned)R), dim3(kRT), 0, stream, x, t.a, t.b,
                       t.lam, t.lam_per_row, loss, lse, bad, C, ignore_index, eps, z);
  }
}

template <typename T>
void launch_backward(const at::Tensor& logits, const Mixed& t, const float* lse, const float* g, const float* count,
                     at::Tensor& d, int64_t ignore_index, float eps, float z, int g_per_row, hipStream_t stream) {
  const int64_t R = logits.size(0);
  const int C = (int)logits.size(1);
  const T* x = reinterpret_cast<const T*>(logits.data_ptr());
  T* dx = reinterpret_cast<T*>(d.data_ptr());
  if (C <= kNarrowMax) {
    const dim3 grid((unsigned)((R + kRowsPerBlock - 1) / kRowsPerBlock));
#define XDDP_NARROW_BWD(N)                                                                                     \
  case N:                                                                                                      \
    hipLaunchKernelGGL((xent_mixed_narrow_bwd_kernel<T, N>), grid, dim3(kRT), 0, stream, x, t.a, t.b, t.lam,   \
                       t.lam_per_row, lse, g, count, dx, R, C, ignore_index, eps, z, g_per_row);               \
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
    hipLaunchKernelGGL((xent_mixed_wide_bwd_kernel<T>), dim3((unsigned)R), dim3(kRT), 0, stream, x, t.a, t.b, t.lam,
                       t.lam_per_row, lse, g, count, dx, C, ignore_index, eps, z, g_per_row);
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

// The outputs of cross_entropy_rows_forward for the two-label target (a, b, lam): {loss per row
// fp32 [R], lse per row fp32 [R]} and, for sum and mean, {reduced loss fp32 [], kept-row count (at
// least 1) fp32 [1]}. No launch when R == 0.
std::vector<at::Tensor> cross_entropy_mixed_forward(const at::Tensor& logits, const at::Tensor& a,
                                                    const at::Tensor& b, const at::Tensor& lam, int64_t ignore_index,
                                                    double label_smoothing, double z_loss, int64_t reduction,
                                                    const at::Tensor& bad) {
  const Mixed t = check_mixed(logits, a, b, lam);
  TORCH_CHECK(bad.is_cuda() && bad.scalar_type() == at::kInt && bad.numel() >= 1 && bad.device() == logits.device(),
              "cross_entropy_mixed: bad-target flag must be an int32 tensor on the logits' device");
  TORCH_CHECK(label_smoothing >= 0.0 && label_smoothing < 1.0 && z_loss >= 0.0 && reduction >= 0 && reduction <= 2,
              "cross_entropy_mixed: need 0 <= label_smoothing < 1, z_loss >= 0 and reduction in {0, 1, 2}");
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
                     launch_forward<T>(logits, t, loss.data_ptr<float>(), lse.data_ptr<float>(), bad.data_ptr<int>(),
                                       ignore_index, (float)label_smoothing, (float)z_loss, stream))
  XDDP_HIP_CHECK(hipGetLastError());
  if (reduction == 0) return {loss, lse};
  auto reduced = at::empty({}, f32);
  auto count = at::empty({1}, f32);
  hipLaunchKernelGGL(xent_mixed_finalize_kernel, dim3(1), dim3(kRT), 0, stream, loss.data_ptr<float>(), t.a, t.b,
                     reduced.data_ptr<float>(), count.data_ptr<float>(), R, ignore_index, reduction == 2 ? 1 : 0);
  XDDP_HIP_CHECK(hipGetLastError());
  return {loss, lse, reduced, count};
}

// dlogits (the logits' dtype); g fp32 [1] (sum, mean) or [R] (none), count fp32 [1] for mean
at::Tensor cross_entropy_mixed_backward(const at::Tensor& logits, const at::Tensor& a, const at::Tensor& b,
                                        const at::Tensor& lam, const at::Tensor& lse, const at::Tensor& g,
                                        const c10::optional<at::Tensor>& count, int64_t ignore_index,
                                        double label_smoothing, double z_loss) {
  const Mixed t = check_mixed(logits, a, b, lam);
  const int64_t R = logits.size(0);
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat && lse.numel() == R && lse.is_contiguous(),
              "cross_entropy_mixed_backward: lse must be fp32 [rows] on the device");
  TORCH_CHECK(g.is_cuda() && g.scalar_type() == at::kFloat && g.is_contiguous() && (g.numel() == 1 || g.numel() == R),
              "cross_entropy_mixed_backward: g must be fp32 [1] or [rows] on the device");
  TORCH_CHECK(!count.has_value() ||
                  (count->is_cuda() && count->scalar_type() == at::kFloat && count->numel() == 1 && g.numel() == 1),
              "cross_entropy_mixed_backward: count must be fp32 [1] on the device, with a single g");
  auto d = at::empty_like(logits);
  if (R == 0) return d;
  auto stream = c10::hip::getCurrentHIPStream(logits.device().index()).stream();
  const float* cnt = count.has_value() ? count->data_ptr<float>() : nullptr;
  XDDP_XENT_DISPATCH(logits.scalar_type(),
                     launch_backward<T>(logits, t, lse.data_ptr<float>(), g.data_ptr<float>(), cnt, d, ignore_index,
                                        (float)label_smoothing, (float)z_loss, g.numel() != 1 ? 1 : 0, stream))
  XDDP_HIP_CHECK(hipGetLastError());
  return d;
}

}  // namespace kernels
}  // namespace xddp
