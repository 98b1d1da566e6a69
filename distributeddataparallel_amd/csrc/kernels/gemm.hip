// Dense bf16 GEMM for the transformer linear layers (ViT-L/16, Llama-3-8B forward projections):
//
//   Y[M, N] = epilogue( A[M, K] · B[N, K]ᵀ )      (torch.nn.Linear: A = activations, B = weight)
//
// with the epilogues that otherwise cost an HBM pass each: + bias, + bias -> GELU (writing both
// the pre-activation the backward needs and the activation), + residual (beta = 1 accumulate).
//
// Structure (gfx950, CDNA4): one 256 x BN block tile per CU (8 waves = 2 (M) x 4 (N), each wave a
// 128 x BN/4 sub-tile = 8 x BN/64 MFMA accumulators of mfma_f32_16x16x32_bf16), BK = 64. Both
// operands go global -> LDS with global_load_lds_dwordx4 (LDS-DMA, no VGPR round trip); each
// wave-instruction fills 8 full 128-B rows, the per-lane SOURCE address is pre-swizzled so the
// lane-linear LDS image has the XOR-swizzled chunk order the ds_read_b128 fragment reads want
// (conflict-free column-slice reads). Two LDS stages of 64 KB; each K-tile runs as four
// 16-MFMA phases whose fragment reads are issued one phase ahead, and the DMA of tile k+2 goes
// out at the one `s_waitcnt vmcnt(0)` + raw s_barrier of tile k, halfway through it (details at
// the loop); nothing else drains the pipeline (all LDS in one dynamic array, no other global
// loads in the loop). The MFMA computes the
// transposed tile (B rows as the first operand), so a lane's four accumulators are four
// consecutive output columns of one row: the C tile goes to LDS as 8-B writes and leaves as full
// 16-B row chunks, where the epilogue math runs. Block ids are remapped XCD-contiguously and
// each XCD's concurrent tiles form a GM x (32 / GM) block that shares A and B panels in its L2.
// Rows past M re-read row M - 1 and are not stored.
//
// The pipeline (tile geometry and order, DMA layout, K loop, C tile stage, tile-width choice) is
// gemm_pipeline.h, shared with gemm_fp8.hip; this file holds the bf16 operand traits, the three
// MODEs' source addressing, the six epilogues and the host entry points.
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include "common.h"
#include "kernels/dev_utils.h"
#include "kernels/gemm_pipeline.h"
#include "kernels/norm.h"

namespace xddp {
namespace kernels {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kBK = 64;  // elements per K-tile: the pipeline's 128-B LDS row

// Operand traits of the shared K loop (gemm_pipeline.h): a fragment is the eight bf16 of one 16-B
// chunk, two k-halves per K-tile, so a pair costs two mfma_f32_16x16x32_bf16.
struct Bf16Ops {
  using Frag = bf16x8;
  static constexpr int kSteps = 2;
  template <int H>
  static __device__ __forceinline__ void pack(Frag (&f)[2][H], const u32x4 (&c)[2][H]) {
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int i = 0; i < H; ++i) f[kh][i] = __builtin_bit_cast(bf16x8, c[kh][i]);
  }
  static __device__ __forceinline__ f32x4 mfma(bf16x8 b, bf16x8 a, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, c, 0, 0, 0);
  }
};

enum Epi : int { kEpiNone = 0, kEpiBias = 1, kEpiBiasGelu = 2, kEpiResidual = 3, kEpiDGelu = 4, kEpiStats = 5 };

// CONV: A is not a matrix but the implicit im2col of a 3x3 pad-1 convolution (NHWC bf16 input
// [B, IH, IW, C], weights OHWI [N][3][3][C] = B[N, 9C]): row m = output pixel (b, oh, ow), K-tile
// kt = tap (kt / (C/64)) x 64-channel block; the DMA source of a row is the input pixel under
// that tap, or a zero line for padding taps (no branch). Same pipeline as the dense GEMM; this is
// the ResNet-50 3x3 forward / stride-1 input gradient for N >= 256, where the 4-phase loop beats
// the 3-stage conv3x3.hip kernel (scripts/conv3x3_ceiling.py).
//
// DGS2 (MODE 2): the input gradient of a stride-2 3x3 pad-1 convolution as four phase GEMMs in one
// launch. dX pixel (2i + ph, 2j + pw) only receives the taps whose stride-2 window lands on it:
// with the 180-degree-rotated weight wr[ci][a][b][co] = w[co][2-a][2-b][ci],
//   dX[2i+ph][2j+pw] = sum over a in A(ph), b in A(pw) of dY[i + r(a)][j + s(b)] · wr[a][b]
// where A(0) = {1} (offset 0) and A(1) = {0 (offset 0), 2 (offset +1)}: phases of 1, 2, 2 and 4
// taps, K = taps x Cout. Row m of phase p = dY-grid pixel (b, i, j); its K-tiles DMA the dY pixels
// under the phase's taps (zero line past the bottom / right edge) and the matching Cout block of
// wr's tap (B = wr viewed [Cin, 9 Cout], ldb = 9 Cout); the C tile is written straight to the
// strided dX pixels — every dX pixel exactly once, no zero-fill, no scatter pass. Blocks are
// phase-major, heaviest phase first (4 taps, then the two 2-tap phases, then the 1-tap one), and
// the XCD remap / grouped tile order run inside each phase.
struct ConvGeo {
  int IH, IW, OH, OW, stride, C;
  const uint16_t* zeros;
  int XH = 0, XW = 0;  // DGS2: dX spatial size (even); IH/IW = OH/OW = the dY grid
};

constexpr int kModeDense = 0, kModeConv = 1, kModeDgS2 = 2;

template <int BN, int EPI, int MODE = kModeDense>
__global__ __launch_bounds__(kThreads, 1) void gemm_nt_kernel(const uint16_t* __restrict__ A,
                                                              const uint16_t* __restrict__ B,
                                                              uint16_t* Y, uint16_t* __restrict__ Y2,
                                                              const uint16_t* __restrict__ bias,
                                                              const uint16_t* res, float* __restrict__ part,
                                                              int M, int N, int K, int ntiles, int64_t ldr,
                                                              ConvGeo cg) {
  using Geo = TileGeo<BN>;
  constexpr int AI = Geo::AI, BI = Geo::BI, STAGE = Geo::STAGE;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

  constexpr bool CONV = MODE != kModeDense;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // DGS2: phase-major blocks (heaviest first), each phase a full M x N tile grid
  const int tiles = MODE == kModeDgS2 ? gridDim.x / 4 : gridDim.x;
  const int pidx = MODE == kModeDgS2 ? blockIdx.x / tiles : 0;
  const int ph = pidx == 0 || pidx == 2, pw = pidx <= 1;  // phase order (1,1) (0,1) (1,0) (0,0)
  const TileOrigin org = tile_origin<BN>(blockIdx.x - pidx * tiles, tiles, ntiles);
  const int mt = org.mt, n0 = org.nt * BN, m0 = mt * kBM;
  // DGS2: the phase's tap count (1 << (ph + pw)) times the Cout blocks; ldb = 9 Cout
  const int nk = MODE == kModeDgS2 ? ((cg.C / kBK) << (ph + pw)) : K / kBK;
  const int ldb = MODE == kModeDgS2 ? 9 * cg.C : K;

  // DMA sources (layout: gemm_pipeline.h): the offsets are recomputed per issue from two per-lane
  // values (few live VGPRs: the 4-phase loop needs ~224 for accumulators and fragments). Rows past
  // M re-read row M - 1 (never stored).
  const int drow = dma_row(lane, wid);                 // + i * 8 NW (A, i < AI) / j * 8 NW (B)
  const int dchunk = 8 * dma_src_chunk(lane, drow);  // in elements
  // CONV: per A row, the top-left input pixel of its 3x3 window (packed (ih0 + 2) << 16 | (iw0 + 2))
  // and that pixel's element offset (may point before the row for padding windows; never
  // dereferenced then). Host-checked: the input has < 2^31 elements.
  int vmask[CONV ? AI : 1], cbase[CONV ? AI : 1];  // CONV: taps inside the image (bit t), window offset
  if constexpr (MODE == kModeDgS2) {
    // row = dY-grid pixel (b, i, j); tap t of the phase reads dY (i + r_t, j + s_t), r_t, s_t in {0, 1}
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      const int row = min(m0 + drow + i * 8 * NW, M - 1);
      const int hw = cg.OH * cg.OW, b = row / hw, rem = row - b * hw, y = rem / cg.OW, x = rem - y * cg.OW;
      int m = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int r = ph ? (t >> pw) : 0, sx = pw ? (t & 1) : 0;
        m |= (y + r < cg.IH && x + sx < cg.IW) << t;
      }
      vmask[i] = m;
      cbase[i] = ((b * cg.IH + y) * cg.IW + x) * cg.C + dchunk;
    }
  } else if constexpr (CONV) {
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      const int row = min(m0 + drow + i * 8 * NW, M - 1);
      const int hw = cg.OH * cg.OW, b = row / hw, rem = row - b * hw, oh = rem / cg.OW, ow = rem - oh * cg.OW;
      const int st = cg.stride & 0xffff, ih0 = oh * st - 1, iw0 = ow * st - 1;
      int m = 0;
#pragma unroll
      for (int t = 0; t < 9; ++t)
        m |= ((unsigned)(ih0 + t / 3) < (unsigned)cg.IH && (unsigned)(iw0 + t % 3) < (unsigned)cg.IW) << t;
      vmask[i] = m;
      cbase[i] = ((b * cg.IH + ih0) * cg.IW + iw0) * cg.C + dchunk;
    }
  }
  auto issue = [&](int kt, int buf) {
    uint8_t* As = smem + buf * STAGE;
    int boff = kt * kBK;  // B's K offset (DGS2: the tap's block of wr)
    if constexpr (MODE == kModeDgS2) {
      const int lg = cg.stride >> 16, tap = kt >> lg, cb = kt & ((1 << lg) - 1);
      const int tr = pw ? tap >> 1 : tap, tc = pw ? tap & 1 : 0;  // row / column tap of the phase
      const int r = ph ? tr : 0, sx = pw ? tc : 0, a = ph ? 2 * tr : 1, bb = pw ? 2 * tc : 1;
      const int toff = (r * cg.IW + sx) * cg.C + cb * kBK;
      boff = (a * 3 + bb) * cg.C + cb * kBK;
#pragma unroll
      for (int i = 0; i < AI; ++i) {
        const bool ok = (vmask[i] >> tap) & 1;
        const uint16_t* src = ok ? A + (cbase[i] + toff) : cg.zeros;
        __builtin_amdgcn_global_load_lds((const void*)src, (lds_ptr_t)(As + (wid * 8 + i * 8 * NW) * 128), 16, 0, 0);
      }
    } else if constexpr (CONV) {
      // C / 64 is a power of two (host-checked): cg.stride's high half carries its log2
      const int lg = cg.stride >> 16, tap = kt >> lg, cb = kt & ((1 << lg) - 1), r = (tap * 11) >> 5, sx = tap - 3 * r;
      const int toff = (r * cg.IW + sx) * cg.C + cb * kBK;
#pragma unroll
      for (int i = 0; i < AI; ++i) {
        const bool ok = (vmask[i] >> tap) & 1;
        const uint16_t* src = ok ? A + (cbase[i] + toff) : cg.zeros;
        __builtin_amdgcn_global_load_lds((const void*)src, (lds_ptr_t)(As + (wid * 8 + i * 8 * NW) * 128), 16, 0, 0);
      }
    } else {
#pragma unroll
      for (int i = 0; i < AI; ++i) {
        const int row = min(m0 + drow + i * 8 * NW, M - 1);
        const uint16_t* src = A + (uint32_t)row * (uint32_t)K + (uint32_t)(dchunk + kt * kBK);
        __builtin_amdgcn_global_load_lds((const void*)src, (lds_ptr_t)(As + (wid * 8 + i * 8 * NW) * 128), 16, 0, 0);
      }
    }
    uint8_t* Bs = As + kBM * 128;
#pragma unroll
    for (int j = 0; j < BI; ++j) {
      const uint16_t* src = B + (uint32_t)(n0 + drow + j * 8 * NW) * (uint32_t)ldb + (uint32_t)(dchunk + boff);
      __builtin_amdgcn_global_load_lds((const void*)src, (lds_ptr_t)(Bs + (wid * 8 + j * 8 * NW) * 128), 16, 0, 0);
    }
  };

  f32x4 acc[Geo::TM][Geo::TN];
#pragma unroll
  for (int i = 0; i < Geo::TM; ++i)
#pragma unroll
    for (int j = 0; j < Geo::TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  k_loop_4phase<BN, Bf16Ops>(tid, nk, acc, issue);

  // ---- epilogue: fp32 -> bf16 C tile through LDS, 16-B row chunks out ----
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // every wave is done reading the stages
  constexpr int CST = Geo::CST;
  uint8_t* Cs = smem;
  c_tile_to_lds<BN>(Cs, tid, acc, [&](f32x4 v, int col) {
    if (EPI == kEpiBias || EPI == kEpiBiasGelu) {  // bias in fp32 before the one rounding
      const uint2 bb = *reinterpret_cast<const uint2*>(bias + n0 + col);
      v[0] += bf(bb.x & 0xffffu);
      v[1] += bf(bb.x >> 16);
      v[2] += bf(bb.y & 0xffffu);
      v[3] += bf(bb.y >> 16);
    }
    return v;
  });

  constexpr int CPR = BN / 8;
  const int cc = readout_col<BN>(tid);  // this thread's 16-B chunk column of the C tile
  const int rows_valid = min(kBM, M - m0);
  u32x4 rb{};
  if (EPI == kEpiResidual && bias) rb = *reinterpret_cast<const u32x4*>(bias + n0 + cc * 8);
  float csum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // kEpiDGelu: this thread's column sums
  // kEpiStats: per-channel shifted sums (shift = the tile's row 0, always valid) for the following
  // BatchNorm's statistics, as conv3x3.hip's epilogue (csum = sum d, cssq = sum d^2)
  float cssq[EPI == kEpiStats ? 8 : 1], st_n = 0.f;
  u32x4 st_k{};
  if (EPI == kEpiStats) {
#pragma unroll
    for (int e = 0; e < 8; ++e) cssq[e] = 0.f;
    st_k = *reinterpret_cast<const u32x4*>(Cs + cc * 16);
  }
  auto out_row = [&](int row, u32x4 v) {
    int64_t off = (int64_t)(m0 + row) * N + n0 + cc * 8;
    if constexpr (MODE == kModeDgS2) {  // dY-grid pixel (b, i, j) -> dX pixel (b, 2i + ph, 2j + pw)
      const int m = m0 + row, hw = cg.OH * cg.OW, b = m / hw, rem = m - b * hw, y = rem / cg.OW, x = rem - y * cg.OW;
      off = (((int64_t)b * cg.XH + 2 * y + ph) * cg.XW + 2 * x + pw) * N + n0 + cc * 8;
    }
    if (EPI == kEpiBiasGelu) {
      *reinterpret_cast<u32x4*>(Y + off) = v;  // pre-activation (the backward's dGELU input)
      u32x4 g;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        g[e] = dev::pack_bf16x2(dev::gelu(bf(v[e] & 0xffffu)), dev::gelu(bf(v[e] >> 16)));
      *reinterpret_cast<u32x4*>(Y2 + off) = g;
    } else if (EPI == kEpiDGelu) {
      // dh = (g·W, the bf16 C tile) · gelu'(h) in fp32; the fp32 dh also feed the column sums
      const u32x4 hv = *reinterpret_cast<const u32x4*>(res + (int64_t)(m0 + row) * ldr + n0 + cc * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float lo = bf(v[e] & 0xffffu) * dev::gelu_grad(bf(hv[e] & 0xffffu));
        const float hi = bf(v[e] >> 16) * dev::gelu_grad(bf(hv[e] >> 16));
        csum[2 * e] += lo;
        csum[2 * e + 1] += hi;
        v[e] = dev::pack_bf16x2(lo, hi);
      }
      *reinterpret_cast<u32x4*>(Y + off) = v;
    } else if (EPI == kEpiStats) {
      __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(Y + off));
      st_n += 1.f;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const float d0 = bf(v[h] & 0xffffu) - bf(st_k[h] & 0xffffu);
        const float d1 = bf(v[h] >> 16) - bf(st_k[h] >> 16);
        csum[2 * h] += d0;
        csum[2 * h + 1] += d1;
        cssq[2 * h] = fmaf(d0, d0, cssq[2 * h]);
        cssq[2 * h + 1] = fmaf(d1, d1, cssq[2 * h + 1]);
      }
    } else if (EPI == kEpiResidual) {
      // y = res + (A·Bᵀ, already rounded to bf16 in the C tile) [+ bias]: one extra rounding of
      // the product against addmm_'s single one (the residual term dominates the sum)
      const u32x4 r = *reinterpret_cast<const u32x4*>(res + (int64_t)(m0 + row) * ldr + n0 + cc * 8);
      if (bias) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          v[e] = dev::pack_bf16x2(bf(r[e] & 0xffffu) + bf(v[e] & 0xffffu) + bf(rb[e] & 0xffffu),
                                  bf(r[e] >> 16) + bf(v[e] >> 16) + bf(rb[e] >> 16));
      } else {
        v = add_bf16x8(r, v);
      }
      *reinterpret_cast<u32x4*>(Y + off) = v;
    } else {
      *reinterpret_cast<u32x4*>(Y + off) = v;
    }
  };
  readout_rows<BN>(Cs, tid, rows_valid, out_row);
  if (EPI == kEpiStats) {
    // lanes sharing cc (xor over the lane bits above log2(CPR)), then the waves through LDS; one
    // (count, mean, M2) per channel and tile, group-minor: part[q][N][mtiles] (bn_stats_from_partials)
#pragma unroll
    for (int o = CPR; o < 64; o <<= 1) {
      st_n += __shfl_xor(st_n, o, 64);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        csum[e] += __shfl_xor(csum[e], o, 64);
        cssq[e] += __shfl_xor(cssq[e], o, 64);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // C tile reads done: reuse smem
    float* red = reinterpret_cast<float*>(smem);                      // [NW][2][BN] sums, [NW][CPR] counts
    float* redn = red + NW * 2 * BN;
    float* redk = redn + NW * CPR;                                    // [BN] the shifts
    if (lane < CPR) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        red[(wid * 2 + 0) * BN + cc * 8 + e] = csum[e];
        red[(wid * 2 + 1) * BN + cc * 8 + e] = cssq[e];
        if (wid == 0) redk[cc * 8 + e] = (e & 1) ? bf(st_k[e >> 1] >> 16) : bf(st_k[e >> 1] & 0xffffu);
      }
      redn[wid * CPR + cc] = st_n;
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    const int G = gridDim.x / ntiles;
    for (int c = tid; c < BN; c += kThreads) {
      float tn = 0.f, ts = 0.f, tss = 0.f;
      for (int w = 0; w < NW; ++w) {
        tn += redn[w * CPR + c / 8];
        ts += red[(w * 2 + 0) * BN + c];
        tss += red[(w * 2 + 1) * BN + c];
      }
      const float mean_s = ts / tn;  // tn >= 1: row 0 is always valid
      part[((int64_t)0 * N + n0 + c) * G + mt] = tn;
      part[((int64_t)1 * N + n0 + c) * G + mt] = redk[c] + mean_s;
      part[((int64_t)2 * N + n0 + c) * G + mt] = fmaxf(tss - ts * mean_s, 0.f);
    }
  }
  if (EPI == kEpiDGelu) {
    // column sums of the tile: the kThreads / CPR row groups meet in LDS past the C tile, then
    // thread c < BN writes part[m-tile][n0 + c] (colsum_partials adds the m-tiles up)
    constexpr int RG = kThreads / CPR;
    float* red = reinterpret_cast<float*>(smem + kBM * CST);
#pragma unroll
    for (int e = 0; e < 8; ++e) red[(tid / CPR) * BN + cc * 8 + e] = csum[e];
    __syncthreads();
    if (tid < BN) {
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < RG; ++r) t += red[r * BN + tid];
      part[(int64_t)mt * N + n0 + tid] = t;
    }
  }
}

template <int BN, int EPI, int MODE = kModeDense>
void launch_gemm(const at::Tensor& a, const at::Tensor& b, uint16_t* y, uint16_t* y2, const uint16_t* bias,
                 const uint16_t* res, float* part, int64_t ldr, int M, int N, int K, hipStream_t stream,
                 const ConvGeo& cg = ConvGeo{}) {
  const int mtiles = (M + kBM - 1) / kBM, ntiles = N / BN, phases = MODE == kModeDgS2 ? 4 : 1;
  // (+ the column-sum exchange of the dGELU epilogue past the C tile)
  const size_t lds = TileGeo<BN>::lds_bytes(EPI == kEpiDGelu ? (size_t)2048 * NW : 0);
  max_dyn_lds_once<gemm_nt_kernel<BN, EPI, MODE>>(lds);
  hipLaunchKernelGGL((gemm_nt_kernel<BN, EPI, MODE>), dim3(phases * mtiles * ntiles), dim3(kThreads), lds, stream,
                     reinterpret_cast<const uint16_t*>(a.data_ptr()), reinterpret_cast<const uint16_t*>(b.data_ptr()),
                     y, y2, bias, res, part, M, N, K, ntiles, ldr, cg);
  XDDP_HIP_CHECK(hipGetLastError());
}

}  // namespace

// a [M, K] bf16 (row-major, rows 16-B aligned), w [N, K] bf16 -> y [M, N] bf16 = a · wᵀ with
// epilogue `epi`: 0 none, 1 + bias, 2 + bias then GELU (returns {pre-activation, activation}),
// 3 + residual (y may be `out` = the residual itself: the in-place x += a·wᵀ of a pre-norm block;
// + bias if given), 4 the GELU backward of an MLP: `residual` is the pre-activation h and the
// result is {dh = (a·wᵀ)·gelu'(h), Σ_rows dh} (the second in bias's dtype if a bias is passed —
// only its dtype is used — else fp32). K % 64 == 0, N % 128 == 0.
std::vector<at::Tensor> gemm_nt(const at::Tensor& a, const at::Tensor& w, const c10::optional<at::Tensor>& bias,
                                int64_t epi, const c10::optional<at::Tensor>& residual,
                                const c10::optional<at::Tensor>& out) {
  TORCH_CHECK(a.is_cuda() && w.is_cuda() && a.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16,
              "gemm_nt: bf16 CUDA operands expected");
  TORCH_CHECK(a.dim() == 2 && w.dim() == 2 && a.size(1) == w.size(1) && a.stride(1) == 1 && a.stride(0) == a.size(1) &&
                  w.is_contiguous(),
              "gemm_nt: a [M, K] and w [N, K] must be contiguous with matching K");
  const int64_t M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(M > 0 && M < (int64_t(1) << 31) && K % 64 == 0 && K > 0 && N % 128 == 0 && N > 0,
              "gemm_nt: needs K % 64 == 0 and N % 128 == 0");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(a.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "gemm_nt: 16-B aligned operands required");
  TORCH_CHECK(epi >= 0 && epi <= 5, "gemm_nt: epi must be 0..5");
  const bool has_bias = bias.has_value() && bias->defined();
  if (has_bias)
    TORCH_CHECK(bias->is_cuda() && bias->scalar_type() == at::kBFloat16 && bias->numel() == N && bias->is_contiguous() &&
                    reinterpret_cast<uintptr_t>(bias->data_ptr()) % 16 == 0,
                "gemm_nt: bias must be a contiguous bf16 [N] vector");
  TORCH_CHECK((epi != 1 && epi != 2) || has_bias, "gemm_nt: epilogues 1 and 2 need a bias");
  at::Tensor res;
  int64_t ldr = N;
  if (epi == 3 || epi == 4) {
    TORCH_CHECK(residual.has_value() && residual->defined(), "gemm_nt: epilogues 3 and 4 need a residual / h");
    res = *residual;
    TORCH_CHECK(res.scalar_type() == at::kBFloat16 && res.dim() == 2 && res.size(0) == M && res.size(1) == N &&
                    res.stride(1) == 1 && res.stride(0) % 8 == 0 && reinterpret_cast<uintptr_t>(res.data_ptr()) % 16 == 0,
                "gemm_nt: residual must be bf16 [M, N] with unit column stride and 16-B aligned rows");
    ldr = res.stride(0);
  }
  at::Tensor y;
  if (out.has_value() && out->defined()) {
    y = *out;
    TORCH_CHECK(y.scalar_type() == at::kBFloat16 && y.dim() == 2 && y.size(0) == M && y.size(1) == N && y.is_contiguous(),
                "gemm_nt: out must be a contiguous bf16 [M, N] tensor");
    TORCH_CHECK(epi < 4, "gemm_nt: epilogues 4 and 5 allocate their outputs");
    TORCH_CHECK(epi != 3 || y.data_ptr() == res.data_ptr() || !(y.data_ptr() < (char*)res.data_ptr() + res.nbytes() &&
                                                                  res.data_ptr() < (char*)y.data_ptr() + y.nbytes()),
                "gemm_nt: out may alias the residual only exactly");
  } else {
    y = at::empty({M, N}, a.options());
  }
  at::Tensor y2 = epi == 2 ? at::empty({M, N}, a.options()) : at::Tensor();
  auto stream = c10::hip::getCurrentHIPStream(a.device().index()).stream();
  const int BN = pick_bn(M, N, cu_count(a.device().index()));
  auto* yp = reinterpret_cast<uint16_t*>(y.data_ptr());
  auto* y2p = epi == 2 ? reinterpret_cast<uint16_t*>(y2.data_ptr()) : nullptr;
  const auto* bp = has_bias ? reinterpret_cast<const uint16_t*>(bias->data_ptr()) : nullptr;
  const auto* rp = (epi == 3 || epi == 4) ? reinterpret_cast<const uint16_t*>(res.data_ptr()) : nullptr;
  at::Tensor part = epi == 4   ? at::empty({(M + kBM - 1) / kBM, N}, a.options().dtype(at::kFloat))
                   : epi == 5 ? at::empty({3, N, (M + kBM - 1) / kBM}, a.options().dtype(at::kFloat))
                              : at::Tensor();
  float* pp = epi >= 4 ? part.data_ptr<float>() : nullptr;
#define XDDP_GEMM(BN_)                                                                                    \
  switch (epi) {                                                                                          \
    case 0: launch_gemm<BN_, kEpiNone>(a, w, yp, y2p, bp, rp, pp, ldr, (int)M, (int)N, (int)K, stream); break;     \
    case 1: launch_gemm<BN_, kEpiBias>(a, w, yp, y2p, bp, rp, pp, ldr, (int)M, (int)N, (int)K, stream); break;     \
    case 2: launch_gemm<BN_, kEpiBiasGelu>(a, w, yp, y2p, bp, rp, pp, ldr, (int)M, (int)N, (int)K, stream); break; \
    case 3: launch_gemm<BN_, kEpiResidual>(a, w, yp, y2p, bp, rp, pp, ldr, (int)M, (int)N, (int)K, stream); break; \
    case 4: launch_gemm<BN_, kEpiDGelu>(a, w, yp, y2p, bp, rp, pp, ldr, (int)M, (int)N, (int)K, stream); break;    \
    default: launch_gemm<BN_, kEpiStats>(a, w, yp, y2p, bp, rp, pp, ldr, (int)M, (int)N, (int)K, stream); break;   \
  }
  if (BN == 256) {
    XDDP_GEMM(256)
  } else {
    XDDP_GEMM(128)
  }
#undef XDDP_GEMM
  if (epi == 2) return {y, y2};
  if (epi == 5) return {y, part};
  if (epi == 4) {
    at::Tensor db = at::empty({N}, has_bias ? bias->options() : a.options().dtype(at::kFloat));
    colsum_partials(part, db);
    return {y, db};
  }
  return {y};
}

// 3x3 pad-1 convolution (stride 1 or 2) on the dense GEMM pipeline (ConvGeo): x [B, C, IH, IW]
// bf16 channels_last, w [N, C, 3, 3] bf16 channels_last (OHWI). Returns {y [B, N, OH, OW]
// channels_last, statistics partials [3, N, mtiles] group-minor (empty without stats)}.
// N % 128 == 0, C % 64 == 0.
std::vector<at::Tensor> conv3x3_gemm(const at::Tensor& x, const at::Tensor& w, int64_t stride, bool stats,
                                     const uint16_t* zeros) {
  const int64_t B = x.size(0), C = x.size(1), IH = x.size(2), IW = x.size(3), N = w.size(0);
  TORCH_CHECK(C % 64 == 0 && N % 128 == 0 && x.numel() < (int64_t(1) << 31), "conv3x3_gemm: unsupported shape");
  const int64_t OH = (IH - 1) / stride + 1, OW = (IW - 1) / stride + 1, M = B * OH * OW;
  auto y = at::empty({B, N, OH, OW}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto stream = c10::hip::getCurrentHIPStream(x.device().index()).stream();
  // 256 x 128 tiles: the 256-wide tile's conv addressing spills ~60 registers past the 256 the
  // 4-phase loop leaves (kernel_resources.py), the 128-wide one fits in 186
  constexpr int BN = 128;
  const int64_t mtiles = (M + kBM - 1) / kBM;
  at::Tensor part = stats ? at::empty({3, N, mtiles}, x.options().dtype(at::kFloat))
                          : at::empty({0}, x.options().dtype(at::kFloat));
  const int lg = __builtin_ctz((unsigned)(C / 64));
  TORCH_CHECK((C / 64) == (int64_t(1) << lg), "conv3x3_gemm: C / 64 must be a power of two");
  // (stride | log2(C / 64) << 16: the kernel splits K-tiles into tap / channel block by shifts)
  const ConvGeo cg{(int)IH, (int)IW, (int)OH, (int)OW, (int)stride | (lg << 16), (int)C, zeros};
  auto* yp = reinterpret_cast<uint16_t*>(y.data_ptr());
  float* pp = stats ? part.data_ptr<float>() : nullptr;
  const int K = (int)(9 * C);
  if (stats) launch_gemm<BN, kEpiStats, kModeConv>(x, w, yp, nullptr, nullptr, nullptr, pp, N, (int)M, (int)N, K, stream, cg);
  else launch_gemm<BN, kEpiNone, kModeConv>(x, w, yp, nullptr, nullptr, nullptr, pp, N, (int)M, (int)N, K, stream, cg);
  return {y, part};
}

// Input gradient of a stride-2 3x3 pad-1 convolution (DGS2, four phase GEMMs in one launch):
// dy [B, Cout, OH, OW] bf16 channels_last, wr = the rotated weight [Cin, Cout, 3, 3] channels_last
// (OHWI memory: wr[ci][a][b][co] = w[co][2-a][2-b][ci], conv3x3_rot_weight) -> dx [B, Cin, XH, XW]
// channels_last with XH = 2 OH, XW = 2 OW (even input sizes). Cin % 128 == 0, Cout / 64 a power of two.
at::Tensor conv3x3_dgrad_s2_gemm(const at::Tensor& dy, const at::Tensor& wr, int64_t XH, int64_t XW,
                                 const uint16_t* zeros) {
  const int64_t B = dy.size(0), Co = dy.size(1), OH = dy.size(2), OW = dy.size(3), Ci = wr.size(0);
  TORCH_CHECK(wr.size(1) == Co && XH == 2 * OH && XW == 2 * OW, "conv3x3_dgrad_s2_gemm: even input sizes only");
  TORCH_CHECK(Co % 64 == 0 && Ci % 128 == 0 && dy.numel() < (int64_t(1) << 31) && B * XH * XW * Ci < (int64_t(1) << 40),
              "conv3x3_dgrad_s2_gemm: unsupported shape");
  const int lg = __builtin_ctz((unsigned)(Co / 64));
  TORCH_CHECK((Co / 64) == (int64_t(1) << lg), "conv3x3_dgrad_s2_gemm: Cout / 64 must be a power of two");
  const int64_t M = B * OH * OW;
  auto dx = at::empty({B, Ci, XH, XW}, dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto stream = c10::hip::getCurrentHIPStream(dy.device().index()).stream();
  ConvGeo cg{(int)OH, (int)OW, (int)OH, (int)OW, 2 | (lg << 16), (int)Co, zeros};
  cg.XH = (int)XH;
  cg.XW = (int)XW;
  launch_gemm<128, kEpiNone, kModeDgS2>(dy, wr, reinterpret_cast<uint16_t*>(dx.data_ptr()), nullptr, nullptr, nullptr,
                                        nullptr, Ci, (int)M, (int)Ci, (int)(4 * Co), stream, cg);
  return dx;
}

}  // namespace kernels
}  // namespace xddp
