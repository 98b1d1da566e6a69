// Mixup / CutMix of an image batch x [B, C, H, W] (fp32 / bf16 / fp16, dense NCHW or NHWC) with a
// partner sample j = partner[i] (default: the flip B - 1 - i), out of place:
//
//   box (y0, y1, x0, x1) not empty   out[i] = x[j] inside the box, x[i] outside   (a copy: bitwise)
//   box empty                        out[i] = lam x[i] + (1 - lam) x[j]           (fp32, one rounding)
//
// lam == 1 copies x[i] and lam == 0 copies x[j] (a weight of exactly 0 contributes nothing, so an
// inf or NaN in the other operand does not leak). lam (fp32, 1 or B elements) and box (int32
// [1, 4] or [B, 4]) are read from device memory: a captured launch sees what was written before
// each replay.
//
// Both memory formats are "rows of L contiguous elements, of which [r0, r1) comes from the partner
// when the row's h = row % H lies in [y0, y1)": NCHW has C·H rows with L = W and the range
// [x0, x1), NHWC has H rows with L = W·C and the range [x0·C, x1·C). A sample is one block row of
// the grid (blockIdx.y), so lam, the box and the partner are block-uniform; a thread takes 8
// consecutive elements of the sample with 16-B loads and stores, finds their row and column with
// one division per 8 elements and walks on from there. A group wholly outside the box reads only
// x[i], one wholly inside only x[j]. Where the base address or the sample size (C·H·W % 8 != 0)
// rules out 16-B access, the scalar kernel does the same per element.
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include "common.h"
#include "kernels/dev_utils.h"

namespace xddp {
namespace kernels {

namespace {

constexpr int kMT = 256;  // threads per block
constexpr int kMU = 2;    // groups of 8 elements per thread

struct Plan {
  int j;         // partner sample
  float lam;
  bool cut;      // box not empty
  int y0, y1, r0, r1;
};

// out-of-range partners fall back to the sample itself (never a read outside x)
__device__ __forceinline__ Plan read_plan(int i, int B, const int* partner, const float* lam, int lam_per_sample,
                                          const int* box, int box_per_sample, int rmul) {
  Plan p;
  p.j = partner != nullptr ? partner[i] : B - 1 - i;
  if (p.j < 0 || p.j >= B) p.j = i;
  p.lam = lam[lam_per_sample ? i : 0];
  const int* b = box + (box_per_sample ? 4 * i : 0);
  p.y0 = b[0];
  p.y1 = b[1];
  const int x0 = b[2], x1 = b[3];
  p.cut = p.y1 > p.y0 && x1 > x0;
  p.r0 = x0 * rmul;
  p.r1 = x1 * rmul;
  return p;
}

__device__ __forceinline__ float blend(float lam, float a, float b) { return fmaf(lam, a, (1.f - lam) * b); }

template <typename T>
__global__ __launch_bounds__(kMT) void mix_scalar_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                         const int* __restrict__ partner,
                                                         const float* __restrict__ lam, int lam_per_sample,
                                                         const int* __restrict__ box, int box_per_sample, int B,
                                                         unsigned N, unsigned L, unsigned H, int rmul) {
  const int i = blockIdx.y;
  const Plan p = read_plan(i, B, partner, lam, lam_per_sample, box, box_per_sample, rmul);
  const T* xi = x + (int64_t)i * N;
  const T* xj = x + (int64_t)p.j * N;
  T* o = out + (int64_t)i * N;
  for (unsigned e = blockIdx.x * kMT + threadIdx.x; e < N; e += gridDim.x * kMT) {
    if (p.cut) {
      const unsigned row = e / L;
      const int col = (int)(e - row * L), h = (int)(row % H);
      const bool in = h >= p.y0 && h < p.y1 && col >= p.r0 && col < p.r1;
      o[e] = in ? xj[e] : xi[e];
    } else if (p.lam == 1.f) {
      o[e] = xi[e];
    } else if (p.lam == 0.f) {
      o[e] = xj[e];
    } else {
      dev::Elem<T, float>::st(o, e, blend(p.lam, dev::Elem<T, float>::ld(xi, e), dev::Elem<T, float>::ld(xj, e)));
    }
  }
}

// 8 elements as raw bits: one 16-B word group for the 2-byte types, two for fp32
template <typename T>
struct Raw8 {
  static constexpr int kWords = sizeof(T) * 8 / 16;
  dev::u32x4 w[kWords];
  __device__ __forceinline__ void ld(const T* p) {
#pragma unroll
    for (int k = 0; k < kWords; ++k) w[k] = reinterpret_cast<const dev::u32x4*>(p)[k];
  }
  __device__ __forceinline__ void st(T* p) const {
#pragma unroll
    for (int k = 0; k < kWords; ++k) reinterpret_cast<dev::u32x4*>(p)[k] = w[k];
  }
  // element k from `other` where bit k of mask is set
  __device__ __forceinline__ void take(const Raw8& other, unsigned mask) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (mask >> k & 1u) w[k / 4][k % 4] = other.w[k / 4][k % 4];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t m = (mask >> (2 * k) & 1u ? 0x0000ffffu : 0u) | (mask >> (2 * k + 1) & 1u ? 0xffff0000u : 0u);
        w[0][k] = (other.w[0][k] & m) | (w[0][k] & ~m);
      }
    }
  }
};

template <typename T>
__global__ __launch_bounds__(kMT) void mix_vec_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                      const int* __restrict__ partner, const float* __restrict__ lam,
                                                      int lam_per_sample, const int* __restrict__ box,
                                                      int box_per_sample, int B, unsigned N, unsigned L, unsigned H,
                                                      int rmul) {
  const int i = blockIdx.y;
  const Plan p = read_plan(i, B, partner, lam, lam_per_sample, box, box_per_sample, rmul);
  const T* xi = x + (int64_t)i * N;
  const T* xj = x + (int64_t)p.j * N;
  T* o = out + (int64_t)i * N;
  const unsigned nvec = N / 8;  // N % 8 == 0 (host)
  const unsigned v0 = (blockIdx.x * kMU) * kMT + threadIdx.x;
  if (p.cut) {
#pragma unroll
    for (int u = 0; u < kMU; ++u) {
      const unsigned v = v0 + u * kMT;
      if (v >= nvec) break;
      const unsigned e = v * 8;
      const unsigned row = e / L;
      unsigned col = e - row * L, h = row % H;
      unsigned mask = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const bool in = (int)h >= p.y0 && (int)h < p.y1 && (int)col >= p.r0 && (int)col < p.r1;
        mask |= in ? 1u << k : 0u;
        if (++col == L) {
          col = 0;
          if (++h == H) h = 0;
        }
      }
      Raw8<T> a;
      if (mask == 0xffu) {
        a.ld(xj + e);
      } else {
        a.ld(xi + e);
        if (mask != 0u) {
          Raw8<T> b;
          b.ld(xj + e);
          a.take(b, mask);
        }
      }
      a.st(o + e);
    }
  } else if (p.lam == 1.f || p.lam == 0.f) {
    const T* src = p.lam == 1.f ? xi : xj;
#pragma unroll
    for (int u = 0; u < kMU; ++u) {
      const unsigned v = v0 + u * kMT;
      if (v >= nvec) break;
      Raw8<T> a;
      a.ld(src + v * 8);
      a.st(o + v * 8);
    }
  } else {
#pragma unroll
    for (int u = 0; u < kMU; ++u) {
      const unsigned v = v0 + u * kMT;
      if (v >= nvec) break;
      float a[8], b[8];
      dev::Vec8<T>::ld(xi + v * 8, a);
      dev::Vec8<T>::ld(xj + v * 8, b);
#pragma unroll
      for (int k = 0; k < 8; ++k) a[k] = blend(p.lam, a[k], b[k]);
      dev::Vec8<T>::st(o + v * 8, a);
    }
  }
}

template <typename T>
void launch_mix(const at::Tensor& x, at::Tensor& out, const int* partner, const float* lam, int lam_per_sample,
                const int* box, int box_per_sample, int B, unsigned N, unsigned L, unsigned H, int rmul,
                hipStream_t stream) {
  const T* xp = reinterpret_cast<const T*>(x.data_ptr());
  T* op = reinterpret_cast<T*>(out.data_ptr());
  const bool vec = N % 8 == 0 && reinterpret_cast<uintptr_t>(xp) % 16 == 0 && reinterpret_cast<uintptr_t>(op) % 16 == 0;
  if (vec) {
    const unsigned per_block = kMT * kMU * 8;
    const dim3 grid((N + per_block - 1) / per_block, (unsigned)B);
    hipLaunchKernelGGL((mix_vec_kernel<T>), grid, dim3(kMT), 0, stream, xp, op, partner, lam, lam_per_sample, box,
                       box_per_sample, B, N, L, H, rmul);
  } else {
    unsigned gx = (N + kMT - 1) / kMT;
    gx = gx > 1024u ? 1024u : gx;
    hipLaunchKernelGGL((mix_scalar_kernel<T>), dim3(gx, (unsigned)B), dim3(kMT), 0, stream, xp, op, partner, lam,
                       lam_per_sample, box, box_per_sample, B, N, L, H, rmul);
  }
}

}  // namespace

at::Tensor mix_images(const at::Tensor& x, const c10::optional<at::Tensor>& partner, const at::Tensor& lam,
                      const at::Tensor& box) {
  const auto st = x.scalar_type();
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && (st == at::kFloat || st == at::kBFloat16 || st == at::kHalf),
              "mix_images: x must be a 4-D fp32 / bf16 / fp16 CUDA tensor [B, C, H, W]");
  const bool nchw = x.is_contiguous();
  TORCH_CHECK(nchw || x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "mix_images: x must be dense in the contiguous or the channels_last memory format");
  const int64_t B = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(B <= 65535 && C * H * W < (int64_t(1) << 31), "mix_images: need B <= 65535 and C * H * W < 2^31");
  TORCH_CHECK(lam.is_cuda() && lam.device() == x.device() && lam.scalar_type() == at::kFloat && lam.is_contiguous() &&
                  (lam.numel() == 1 || lam.numel() == B),
              "mix_images: lam must be fp32 with 1 or B elements on x's device");
  TORCH_CHECK(box.is_cuda() && box.device() == x.device() && box.scalar_type() == at::kInt && box.is_contiguous() &&
                  box.dim() == 2 && box.size(1) == 4 && (box.size(0) == 1 || box.size(0) == B),
              "mix_images: box must be int32 [1, 4] or [B, 4] (y0, y1, x0, x1) on x's device");
  const int* pp = nullptr;
  if (partner.has_value()) {
    TORCH_CHECK(partner->is_cuda() && partner->device() == x.device() && partner->scalar_type() == at::kInt &&
                    partner->is_contiguous() && partner->dim() == 1 && partner->size(0) == B,
                "mix_images: partner must be int32 [B] on x's device");
    pp = partner->data_ptr<int>();
  }
  auto out = at::empty_like(x);  // x is dense: the same strides
  if (x.numel() == 0) return out;
  const unsigned N = (unsigned)(C * H * W);
  const unsigned L = (unsigned)(nchw ? W : W * C);
  const int rmul = nchw ? 1 : (int)C;
  auto stream = c10::hip::getCurrentHIPStream(x.device().index()).stream();
  const int lps = lam.numel() != 1 ? 1 : 0, bps = box.size(0) != 1 ? 1 : 0;
  if (st == at::kFloat)
    launch_mix<float>(x, out, pp, lam.data_ptr<float>(), lps, box.data_ptr<int>(), bps, (int)B, N, L, (unsigned)H, rmul,
                      stream);
  else if (st == at::kBFloat16)
    launch_mix<dev::bf16_t>(x, out, pp, lam.data_ptr<float>(), lps, box.data_ptr<int>(), bps, (int)B, N, L,
                            (unsigned)H, rmul, stream);
  else
    launch_mix<dev::f16_t>(x, out, pp, lam.data_ptr<float>(), lps, box.data_ptr<int>(), bps, (int)B, N, L, (unsigned)H,
                           rmul, stream);
  XDDP_HIP_CHECK(hipGetLastError());
  return out;
}

}  // namespace kernels
}  // namespace xddp
