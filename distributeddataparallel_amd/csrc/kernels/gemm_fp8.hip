// FP8 GEMM for the opt-in FP8 linear layers (ops/fp8.py):
//
//   Y[M, N] = (A[M, K] · B[N, K]ᵀ) / (scale_a · scale_b)   [+ res]      (bf16 out, fp32 accumulate)
//
// A and B are one-byte OCP FP8 operands (e4m3 or e5m2, chosen per operand), quantized per tensor
// by fp8_cast.hip; the two scales are device scalars read once per block.
//
// Structure: gemm.hip's dense pipeline with one-byte elements. 256 x BN block tile (8 waves =
// 2 (M) x 4 (N)), BK = 128 elements, so an LDS row is still 128 B = eight 16-B chunks and the
// LDS-DMA staging with pre-swizzled source addresses, the XOR-swizzled fragment reads, the
// two-stage / four-phase K loop, the XCD-grouped tile order and the C tile through LDS carry over
// unchanged. The MFMA is the block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 with both block
// scales the constant E8M0 value 127 (= 1.0): one instruction per (A fragment, B fragment) and
// K-tile where the bf16 kernel issues two 16x16x32.
//
// Operand layout: a lane's 32-byte operand is the two 16-B chunks (lane >> 4) and 4 + (lane >> 4)
// of row (lane & 15) — the same two ds_read_b128 per fragment as the bf16 kernel's two k-halves.
// With unit block scales a dot product does not depend on the order of K as long as both operands
// use the same order, and A and B fragments are loaded with the same lane-to-bytes mapping; the
// four lane groups cover disjoint quarters of the K step. tests/test_gemm_fp8_gpu.py checks this
// with exact integer data.
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <type_traits>

#include "common.h"
#include "kernels/dev_utils.h"
#include "kernels/norm.h"

namespace xddp {
namespace kernels {

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));
using dev::f32x4;
using dev::u32x4;
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr int kBM = 256, kBK = 128, kWM = 2, kWN = 4, NW = kWM * kWN, kThreads = 64 * NW;
constexpr int kScaleOne = 0x7f7f7f7f;  // E8M0 127 = 2^0 in every byte: any op_sel picks 1.0

__device__ __forceinline__ float bf(uint32_t bits16) { return __uint_as_float(bits16 << 16); }

// AF / BF: 0 = e4m3, 1 = e5m2 (the MFMA's format codes for 8-bit operands)
template <int BN, int AF, int BF>
__global__ __launch_bounds__(kThreads, 1) void gemm_fp8_nt_kernel(const uint8_t* __restrict__ A,
                                                                  const uint8_t* __restrict__ B, uint16_t* Y,
                                                                  const uint16_t* res, const float* __restrict__ sa,
                                                                  const float* __restrict__ sb, int M, int N, int K,
                                                                  int ntiles, int64_t ldr) {
  constexpr int AI = kBM / 8 / NW, BI = BN / 8 / NW;  // DMA wave-instructions per stage (8 rows each)
  static_assert(AI * NW * 8 == kBM && BI * NW * 8 == BN, "tile rows must split evenly over the waves");
  constexpr int WTM = kBM / kWM, WTN = BN / kWN, TM = WTM / 16, TN = WTN / 16;
  constexpr int STAGE = (kBM + BN) * 128;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid / kWN, wn = wid % kWN;
  // tile order as gemm.hip: XCD-contiguous runs of logical tiles, GM m-tiles per group
  constexpr int GM = BN == 256 ? 8 : 4;
  const int tiles = gridDim.x;
  const int wg = dev::xcd_remap(blockIdx.x, tiles);
  const int mtiles = tiles / ntiles, grp = wg / (GM * ntiles), first_m = grp * GM;
  const int gm = min(mtiles - first_m, GM), local = wg - grp * GM * ntiles;
  const int mt = first_m + local % gm, nt = local / gm;
  const int n0 = nt * BN, m0 = mt * kBM;
  const int pos = lane & 7;  // 16-B slot this lane fills in its 128-B LDS row
  const int nk = K / kBK;

  // DMA sources: lane l of wave w fills 16-B slot (l & 7) of rows (w*AI + i)*8 + (l >> 3) with the
  // source chunk pos ^ ((row >> 1) & 7). Rows past M re-read row M - 1 (never stored). An address
  // is a block-uniform 64-bit base (tile origin + K-tile, in SGPRs) plus a 32-bit per-lane offset
  // inside the tile: AI offsets for A (the M clamp is per row), one for B — few live VGPRs, the
  // 4-phase loop needs ~224 for accumulators and fragments.
  const int drow = wid * 8 + (lane >> 3);
  const int dchunk = 16 * (pos ^ ((drow >> 1) & 7));
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

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  {
    // gemm.hip's 4-phase loop: one phase per quadrant (A half x B half) of the wave's output, the
    // next phase's fragment reads interleaved into this phase's MFMAs, one barrier per K-tile.
    constexpr int HA = TM / 2, HB = TN / 2;
    static_assert(HB >= 1, "B halves need at least one 16-column fragment");
    i32x8 fa0[HA], fa1[HA], fb0[HB], fb1[HB];
    const int ra = wm * WTM + (lane & 15), rb = wn * WTN + (lane & 15);
    uint32_t a_lds[2], b_lds[2];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      a_lds[kh] = ra * 128 + 16 * ((kh * 4 + (lane >> 4)) ^ ((ra >> 1) & 7));
      b_lds[kh] = kBM * 128 + rb * 128 + 16 * ((kh * 4 + (lane >> 4)) ^ ((rb >> 1) & 7));
    }
    auto ld = [&](uint32_t off0, uint32_t off1) {
      const u32x4 lo = *reinterpret_cast<const u32x4*>(smem + off0);
      const u32x4 hi = *reinterpret_cast<const u32x4*>(smem + off1);
      return __builtin_bit_cast(i32x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    };
    auto ldA = [&](i32x8 (&f)[HA], int half, int buf) {
#pragma unroll
      for (int i = 0; i < HA; ++i) {
        const uint32_t o = buf * STAGE + (half * HA + i) * 16 * 128;
        f[i] = ld(o + a_lds[0], o + a_lds[1]);
      }
    };
    auto ldB = [&](i32x8 (&f)[HB], int half, int buf) {
#pragma unroll
      for (int j = 0; j < HB; ++j) {
        const uint32_t o = buf * STAGE + (half * HB + j) * 16 * 128;
        f[j] = ld(o + b_lds[0], o + b_lds[1]);
      }
    };
    // B rows are the MFMA's first operand (its format is cbsz), A rows the second (blgp): the
    // transposed tile, so a lane's four accumulators are four consecutive output columns
    auto mma = [&](const i32x8 (&a)[HA], auto ah, const i32x8 (&b)[HB], auto bh) {
      constexpr int AH = decltype(ah)::value, BHV = decltype(bh)::value;
#pragma unroll
      for (int i = 0; i < HA; ++i)
#pragma unroll
        for (int j = 0; j < HB; ++j)
          acc[AH * HA + i][BHV * HB + j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              b[j], a[i], acc[AH * HA + i][BHV * HB + j], BF, AF, 0, kScaleOne, 0, kScaleOne);
    };
    auto interleave = [&](auto nld) {
      constexpr int NLD = decltype(nld)::value, NM = HA * HB;
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);       // one MFMA (waits for this phase's fragments)
      __builtin_amdgcn_sched_group_barrier(0x100, NLD, 0);     // the next phase's reads
      __builtin_amdgcn_sched_group_barrier(0x008, NM - 1, 0);  // the rest of the MFMAs
      __builtin_amdgcn_sched_barrier(0);
    };
    using LA = std::integral_constant<int, 2 * HA>;  // reads of an A half (two 16-B chunks per fragment)
    using LB = std::integral_constant<int, 2 * HB>;
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    // Tile pairs, branch-free; an odd tile count gets a zero tile in front (FP8 zero bytes are
    // 0.0 in both formats), as in gemm.hip.
    const int odd = nk & 1, nv = nk + odd;
    auto sync = [&](int t) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      issue(min(t + 2, nv - 1) - odd, t & 1);
    };
    if (odd) {
      for (int q = tid; q < STAGE / 16; q += kThreads) reinterpret_cast<u32x4*>(smem)[q] = u32x4{0u, 0u, 0u, 0u};
    } else {
      issue(0, 0);
    }
    issue(1 - odd, 1);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AI + BI) : "memory");  // stage 0 ready, stage 1 in flight
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    ldA(fa0, 0, 0);
    ldB(fb0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    for (int t = 0; t < nv; t += 2) {
      // even tile t (stage 0): enters with A0, B0 of t
      ldB(fb1, 1, 0);
      mma(fa0, I0{}, fb0, I0{});
      interleave(LB{});
      ldA(fa1, 1, 0);
      mma(fa0, I0{}, fb1, I1{});
      interleave(LA{});
      sync(t);
      __builtin_amdgcn_sched_barrier(0);
      ldA(fa0, 0, 1);  // A0 of t + 1
      mma(fa1, I1{}, fb1, I1{});
      interleave(LA{});
      ldB(fb1, 1, 1);  // B1 of t + 1
      mma(fa1, I1{}, fb0, I0{});
      interleave(LB{});
      // odd tile t + 1 (stage 1): enters with A0, B1 of t + 1
      ldB(fb0, 0, 1);
      mma(fa0, I0{}, fb1, I1{});
      interleave(LB{});
      ldA(fa1, 1, 1);
      mma(fa0, I0{}, fb0, I0{});
      interleave(LA{});
      sync(t + 1);
      __builtin_amdgcn_sched_barrier(0);
      ldA(fa0, 0, 0);  // A0 of t + 2
      mma(fa1, I1{}, fb0, I0{});
      interleave(LA{});
      ldB(fb0, 0, 0);  // B0 of t + 2
      mma(fa1, I1{}, fb1, I1{});
      interleave(LB{});
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the trailing re-stage DMAs land before the C tile reuses LDS
  }

  // ---- epilogue: dequantize, fp32 -> bf16 C tile through LDS (rows padded 16 B), 16-B row chunks out ----
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // every wave is done reading the stages
  constexpr int CST = BN * 2 + 16;
  uint8_t* Cs = smem;
  const float inv = 1.f / (sa[0] * sb[0]);  // the per-tensor scales, read here so the K loop holds no extra register
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int row = wm * WTM + i * 16 + (lane & 15);
      const int col = wn * WTN + j * 16 + (lane >> 4) * 4;
      const f32x4 v = acc[i][j] * inv;
      uint2 pk;
      pk.x = dev::pack_bf16x2(v[0], v[1]);
      pk.y = dev::pack_bf16x2(v[2], v[3]);
      *reinterpret_cast<uint2*>(Cs + row * CST + col * 2) = pk;
    }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

  constexpr int CPR = BN / 8;
  static_assert(kThreads % CPR == 0, "readout mapping needs a fixed chunk column per thread");
  const int cc = tid % CPR;
  const int rows_valid = min(kBM, M - m0);
  auto out_row = [&](int row, u32x4 v) {
    const int64_t off = (int64_t)(m0 + row) * N + n0 + cc * 8;
    if (res) {
      // y = res + (the product, already rounded to bf16 in the C tile), as gemm.hip's epilogue 3;
      // res may be Y itself: each 16-B chunk is read and written by this thread only
      const u32x4 r = *reinterpret_cast<const u32x4*>(res + (int64_t)(m0 + row) * ldr + n0 + cc * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        v[e] = dev::pack_bf16x2(bf(r[e] & 0xffffu) + bf(v[e] & 0xffffu), bf(r[e] >> 16) + bf(v[e] >> 16));
    }
    *reinterpret_cast<u32x4*>(Y + off) = v;
  };
  constexpr int NIT = kBM * CPR / kThreads, RSTR = kThreads / CPR, EB = NIT < 4 ? NIT : 4;
  static_assert(kBM * CPR % kThreads == 0, "readout rows must divide evenly over the threads");
#pragma unroll
  for (int i0 = 0; i0 < NIT; i0 += EB) {
    u32x4 vv[EB];
#pragma unroll
    for (int j = 0; j < EB; ++j)
      if (i0 + j < NIT)
        vv[j] = *reinterpret_cast<const u32x4*>(Cs + min(tid / CPR + RSTR * (i0 + j), rows_valid - 1) * CST + cc * 16);
#pragma unroll
    for (int j = 0; j < EB; ++j) {
      const int row = tid / CPR + RSTR * (i0 + j);
      if (i0 + j < NIT && row < rows_valid) out_row(row, vv[j]);
    }
  }
}

template <int BN, int AF, int BF>
void launch_gemm_fp8(const uint8_t* a, const uint8_t* b, uint16_t* y, const uint16_t* res, const float* sa,
                     const float* sb, int64_t ldr, int M, int N, int K, hipStream_t stream) {
  const int mtiles = (M + kBM - 1) / kBM, ntiles = N / BN;
  const size_t lds = std::max<size_t>((size_t)2 * (kBM + BN) * 128, (size_t)kBM * (BN * 2 + 16));  // stages | C tile
  static bool attr = false;
  if (!attr) {
    XDDP_HIP_CHECK(hipFuncSetAttribute((const void*)gemm_fp8_nt_kernel<BN, AF, BF>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr = true;
  }
  hipLaunchKernelGGL((gemm_fp8_nt_kernel<BN, AF, BF>), dim3(mtiles * ntiles), dim3(kThreads), lds, stream, a, b, y, res,
                     sa, sb, M, N, K, ntiles, ldr);
  XDDP_HIP_CHECK(hipGetLastError());
}

// Tile width as gemm.hip's pick_bn: 256 x 256 unless the 256 x 128 grid fills the last round better.
int pick_bn_fp8(int64_t M, int64_t N, int cus) {
  if (N % 256) return 128;
  const int64_t mt = (M + kBM - 1) / kBM;
  const int64_t r256 = (mt * (N / 256) + cus - 1) / cus, r128 = (mt * (N / 128) + cus - 1) / cus;
  return 2.0 * r256 <= 1.15 * r128 ? 256 : 128;
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
  static int cus = 0;
  if (!cus) {
    int v = 0;
    cus = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, a.device().index()) == hipSuccess && v > 0
              ? v : 256;
  }
  const int BN = pick_bn_fp8(M, N, cus);
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
