// FP8 GEMM for the opt-in FP8 linear layers (ops/fp8.py):
//
//   Y[M, N] = (A[M, K] · B[N, K]ᵀ) / (scale_a · scale_b)   [+ res]      (bf16 out, fp32 accumulate)
//
// A and B are one-byte OCP FP8 operands (e4m3 or e5m2, chosen per operand), quantized per tensor
// by fp8_cast.hip; the two scales are device scalars read once per block.
//
// Structure: the 4-phase LDS-DMA pipeline of gemm_pipeline.h (shared with the bf16 gemm.hip) with
// one-byte elements. 256 x BN block tile (8 waves = 2 (M) x 4 (N)), BK = 128 elements, so an LDS
// row is the pipeline's 128 B = eight 16-B chunks and the LDS-DMA staging with pre-swizzled source
// addresses, the XOR-swizzled fragment reads, the two-stage / four-phase K loop, the XCD-grouped
// tile order and the C tile through LDS are the header's. The MFMA is the block-scaled
// v_mfma_scale_f32_16x16x128_f8f6f4 with both block scales the constant E8M0 value 127 (= 1.0):
// one instruction per (A fragment, B fragment) and K-tile where the bf16 kernel issues two
// 16x16x32.
//
// Operand layout: a lane's 32-byte operand is the two 16-B chunks (lane >> 4) and 4 + (lane >> 4)
// of row (lane & 15) — the same two ds_read_b128 per fragment as the bf16 kernel's two k-halves.
// With unit block scales a dot product does not depend on the order of K as long as both operands
// use the same order, and A and B fragments are loaded with the same lane-to-bytes mapping; the
// four lane groups cover disjoint quarters of the K step. tests/test_gemm_fp8_gpu.py checks this
// with exact integer data.
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include "common.h"
#include "kernels/dev_utils.h"
#include "kernels/gemm_pipeline.h"
#include "kernels/norm.h"

namespace xddp {
namespace kernels {

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int kBK = 128;               // elements per K-tile: the pipeline's 128-B LDS row
constexpr int kScaleOne = 0x7f7f7f7f;  // E8M0 127 = 2^0 in every byte: any op_sel picks 1.0

// Operand traits of the shared K loop: a fragment is a row's two 16-B chunks joined, one MFMA per
// pair. AF / BF: 0 = e4m3, 1 = e5m2 (the MFMA's format codes for 8-bit operands); B rows are the
// MFMA's first operand (its format is cbsz), A rows the second (blgp).
template <int AF, int BF>
struct Fp8Ops {
  using Frag = i32x8;
  static constexpr int kSteps = 1;
  template <int H>
  static __device__ __forceinline__ void pack(Frag (&f)[1][H], const u32x4 (&c)[2][H]) {
#pragma unroll
    for (int i = 0; i < H; ++i)
      f[0][i] = __builtin_bit_cast(i32x8, __builtin_shufflevector(c[0][i], c[1][i], 0, 1, 2, 3, 4, 5, 6, 7));
  }
  static __device__ __forceinline__ f32x4 mfma(i32x8 b, i32x8 a, f32x4 c) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(b, a, c, BF, AF, 0, kScaleOne, 0, kScaleOne);
  }
};

template <int BN, int AF, int BF>
__global__ __launch_bounds__(kThreads, 1) void gemm_fp8_nt_kernel(const uint8_t* __restrict__ A,
                                                                  const uint8_t* __restrict__ B, uint16_t* Y,
                                                                  const uint16_t* res, const float* __restrict__ sa,
                                                                  const float* __restrict__ sb, int M, int N, int K,
                                                                  int ntiles, int64_t ldr) {
  using Geo = TileGeo<BN>;
  constexpr int AI = Geo::AI, BI = Geo::BI, STAGE = Geo::STAGE;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const TileOrigin org = tile_origin<BN>(blockIdx.x, gridDim.x, ntiles);
  const int n0 = org.nt * BN, m0 = org.mt * kBM;

  // DMA sources (layout: gemm_pipeline.h). Rows past M re-read row M - 1 (never stored). An address
  // is a block-uniform 64-bit base (tile origin + K-tile, in SGPRs) plus a 32-bit per-lane offset
  // inside the tile: AI offsets for A (the M clamp is per row), one for B — few live VGPRs, the
  // 4-phase loop needs ~224 for accumulators and fragments.
  const int drow = dma_row(lane, wid);
  const int dchunk = 16 * dma_src_chunk(lane, drow);  // in bytes = elements
  uint32_t la[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) la[i] = (uint32_t)(min(drow + i * 8 * NW, M - 1 - m0) * K + dchunk);
  const uint32_t lb = (uint32_t)(drow * K + dchunk);
  const uint8_t* Ab = A + (int64_t)m0 * K;
  const uint8_t* Bb = B + (int64_t)n0 * K;
  auto issue = [&](int kt, int buf) {
    uint8_t* As = smem + buf * STAGE;
    const uint8_t* ak = Ab + kt * kBK;
#pragma unroll
    for (int i = 0; i < AI; ++i)
      __builtin_amdgcn_global_load_lds((const void*)(ak + la[i]), (lds_ptr_t)(As + (wid * 8 + i * 8 * NW) * 128), 16, 0, 0);
    uint8_t* Bs = As + kBM * 128;
#pragma unroll
    for (int j = 0; j < BI; ++j) {
      const uint8_t* bk = Bb + ((int64_t)j * 8 * NW * K + kt * kBK);
      __builtin_amdgcn_global_load_lds((const void*)(bk + lb), (lds_ptr_t)(Bs + (wid * 8 + j * 8 * NW) * 128), 16, 0, 0);
    }
  };

  f32x4 acc[Geo::TM][Geo::TN];
#pragma unroll
  for (int i = 0; i < Geo::TM; ++i)
#pragma unroll
    for (int j = 0; j < Geo::TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  k_loop_4phase<BN, Fp8Ops<AF, BF>>(tid, K / kBK, acc, issue);

  // ---- epilogue: dequantize, fp32 -> bf16 C tile through LDS, 16-B row chunks out ----
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // every wave is done reading the stages
  uint8_t* Cs = smem;
  const float inv = 1.f / (sa[0] * sb[0]);  // the per-tensor scales, read here so the K loop holds no extra register
  c_tile_to_lds<BN>(Cs, tid, acc, [&](f32x4 v, int) { return v * inv; });

  const int cc = readout_col<BN>(tid);  // this thread's 16-B chunk column of the C tile
  readout_rows<BN>(Cs, tid, min(kBM, M - m0), [&](int row, u32x4 v) {
    const int64_t off = (int64_t)(m0 + row) * N + n0 + cc * 8;
    // y = res + (the product, already rounded to bf16 in the C tile), as gemm.hip's epilogue 3;
    // res may be Y itself: each 16-B chunk is read and written by this thread only
    if (res) v = add_bf16x8(*reinterpret_cast<const u32x4*>(res + (int64_t)(m0 + row) * ldr + n0 + cc * 8), v);
    *reinterpret_cast<u32x4*>(Y + off) = v;
  });
}

template <int BN, int AF, int BF>
void launch_gemm_fp8(const uint8_t* a, const uint8_t* b, uint16_t* y, const uint16_t* res, const float* sa,
                     const float* sb, int64_t ldr, int M, int N, int K, hipStream_t stream) {
  const int mtiles = (M + kBM - 1) / kBM, ntiles = N / BN;
  const size_t lds = TileGeo<BN>::lds_bytes();
  max_dyn_lds_once<gemm_fp8_nt_kernel<BN, AF, BF>>(lds);
  hipLaunchKernelGGL((gemm_fp8_nt_kernel<BN, AF, BF>), dim3(mtiles * ntiles), dim3(kThreads), lds, stream, a, b, y, res,
                     sa, sb, M, N, K, ntiles, ldr);
  XDDP_HIP_CHECK(hipGetLastError());
}

bool scalar_f32(const at::Tensor& t) { return t.is_cuda() && t.scalar_type() == at::kFloat && t.numel() == 1; }

}  // namespace

// a [M, K], b [N, K]: contiguous uint8 tensors holding OCP FP8 bytes (a_fmt / b_fmt: 0 e4m3, 1 e5m2),
// scale_a / scale_b: float32[1] device scalars (the factors the operands were multiplied by when
// quantized) -> y [M, N] bf16 = (a · bᵀ) / (scale_a · scale_b); epi 1: + residual [M, N] bf16, which
// may be `out` itself (the in-place y += ...). Any M; N % 128 == 0, K % 128 == 0.
at::Tensor gemm_fp8_nt(const at::Tensor& a, const at::Tensor& b, const at::Tensor& scale_a, const at::Tensor& scale_b,
                       int64_t a_fmt, int64_t b_fmt, int64_t epi, const c10::optional<at::Tensor>& residual,
                       const c10::optional<at::Tensor>& out) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.scalar_type() == at::kByte && b.scalar_type() == at::kByte,
              "gemm_fp8_nt: uint8 (FP8 bytes) CUDA operands expected");
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.is_contiguous() && b.is_contiguous(),
              "gemm_fp8_nt: a [M, K] and b [N, K] must be contiguous matrices");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  TORCH_CHECK(b.size(1) == K, "gemm_fp8_nt: K of a (", K, ") and of b (", b.size(1), ") differ");
  TORCH_CHECK(M > 0, "gemm_fp8_nt: M must be positive, got M = ", M);
  TORCH_CHECK(K > 0 && K % 128 == 0, "gemm_fp8_nt: K must be a positive multiple of 128, got K = ", K);
  TORCH_CHECK(N > 0 && N % 128 == 0, "gemm_fp8_nt: N must be a positive multiple of 128, got N = ", N);
  TORCH_CHECK(M * K < (int64_t(1) << 32) && N * K < (int64_t(1) << 32) && M < (int64_t(1) << 31) - kBM,
              "gemm_fp8_nt: operands of 4 GiB or more are not supported (M = ", M, ", N = ", N, ", K = ", K, ")");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(a.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(b.data_ptr()) % 16 == 0,
              "gemm_fp8_nt: 16-B aligned operands required");
  TORCH_CHECK(scalar_f32(scale_a) && scalar_f32(scale_b), "gemm_fp8_nt: scales must be float32[1] CUDA tensors");
  TORCH_CHECK((a_fmt == 0 || a_fmt == 1) && (b_fmt == 0 || b_fmt == 1), "gemm_fp8_nt: formats are 0 (e4m3) or 1 (e5m2)");
  TORCH_CHECK(epi == 0 || epi == 1, "gemm_fp8_nt: epi must be 0 (none) or 1 (+ residual)");
  at::Tensor res;
  int64_t ldr = N;
  if (epi == 1) {
    TORCH_CHECK(residual.has_value() && residual->defined(), "gemm_fp8_nt: epilogue 1 needs a residual");
    res = *residual;
    TORCH_CHECK(res.is_cuda() && res.scalar_type() == at::kBFloat16 && res.dim() == 2 && res.size(0) == M &&
                    res.size(1) == N && res.stride(1) == 1 && res.stride(0) % 8 == 0 && res.stride(0) >= N &&
                    reinterpret_cast<uintptr_t>(res.data_ptr()) % 16 == 0,
                "gemm_fp8_nt: residual must be bf16 [M, N] with unit column stride and 16-B aligned rows");
    ldr = res.stride(0);
  }
  const auto opts = a.options().dtype(at::kBFloat16);
  at::Tensor y;
  if (out.has_value() && out->defined()) {
    y = *out;
    TORCH_CHECK(y.is_cuda() && y.scalar_type() == at::kBFloat16 && y.dim() == 2 && y.size(0) == M && y.size(1) == N &&
                    y.is_contiguous() && reinterpret_cast<uintptr_t>(y.data_ptr()) % 16 == 0,
                "gemm_fp8_nt: out must be a contiguous, 16-B aligned bf16 [M, N] tensor");
    TORCH_CHECK(epi != 1 || y.data_ptr() == res.data_ptr() ||
                    !(y.data_ptr() < (char*)res.data_ptr() + ((M - 1) * ldr + N) * 2 &&
                      res.data_ptr() < (char*)y.data_ptr() + y.nbytes()),
                "gemm_fp8_nt: out may alias the residual only exactly");
    TORCH_CHECK(epi != 1 || y.data_ptr() != res.data_ptr() || ldr == N,
                "gemm_fp8_nt: an aliasing residual must have out's layout");
  } else {
    y = at::empty({M, N}, opts);
  }
  auto stream = c10::hip::getCurrentHIPStream(a.device().index()).stream();
  const int BN = pick_bn(M, N, cu_count(a.device().index()));
  const auto* ap = reinterpret_cast<const uint8_t*>(a.data_ptr());
  const auto* bp = reinterpret_cast<const uint8_t*>(b.data_ptr());
  auto* yp = reinterpret_cast<uint16_t*>(y.data_ptr());
  const auto* rp = epi == 1 ? reinterpret_cast<const uint16_t*>(res.data_ptr()) : nullptr;
  const float *sa = scale_a.data_ptr<float>(), *sb = scale_b.data_ptr<float>();
#define XDDP_GEMM_FP8(BN_, AF_, BF_) \
  launch_gemm_fp8<BN_, AF_, BF_>(ap, bp, yp, rp, sa, sb, ldr, (int)M, (int)N, (int)K, stream)
#define XDDP_GEMM_FP8_FMT(BN_)                        \
  switch (a_fmt * 2 + b_fmt) {                        \
    case 0: XDDP_GEMM_FP8(BN_, 0, 0); break;          \
    case 1: XDDP_GEMM_FP8(BN_, 0, 1); break;          \
    case 2: XDDP_GEMM_FP8(BN_, 1, 0); break;          \
    default: XDDP_GEMM_FP8(BN_, 1, 1); break;         \
  }
  if (BN == 256) {
    XDDP_GEMM_FP8_FMT(256)
  } else {
    XDDP_GEMM_FP8_FMT(128)
  }
#undef XDDP_GEMM_FP8_FMT
#undef XDDP_GEMM_FP8
  return y;
}

}  // namespace kernels
}  // namespace xddp
