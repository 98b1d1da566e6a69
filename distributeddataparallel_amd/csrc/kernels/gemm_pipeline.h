// The 4-phase LDS-DMA GEMM pipeline shared by gemm.hip (bf16: dense, implicit-im2col conv, DGS2)
// and gemm_fp8.hip (one-byte operands): block-tile geometry and tile order, the LDS-DMA destination
// layout with its source swizzle, the fragment offsets, the K loop, the C tile through LDS and the
// host-side tile-width choice. What differs between the two kernels stays in their files: the
// global source addressing (`issue`), the operand traits (fragment type, its LDS load, the MFMA)
// and the epilogue math on the 16-B row chunks.
//
// Layout: one 256 x BN block tile per CU, 8 waves = 2 (M) x 4 (N), each wave a 128 x BN/4 sub-tile
// of 16 x 16 MFMA accumulators. A K-tile is 128 BYTES of K per row (64 bf16 / 128 fp8), so an LDS
// row is eight 16-B chunks whatever the element type; everything here counts in 16-B chunks and
// the element size is the caller's scale factor. Two LDS stages of (256 + BN) rows.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "kernels/dev_utils.h"

namespace xddp {
namespace kernels {

using dev::bf;
using dev::f32x4;
using dev::u32x4;
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr int kBM = 256, kWM = 2, kWN = 4, NW = kWM * kWN, kThreads = 64 * NW;

template <int BN>
struct TileGeo {
  static constexpr int AI = kBM / 8 / NW, BI = BN / 8 / NW;  // DMA wave-instructions per stage (8 rows each)
  static_assert(AI * NW * 8 == kBM && BI * NW * 8 == BN, "tile rows must split evenly over the waves");
  static constexpr int WTM = kBM / kWM, WTN = BN / kWN, TM = WTM / 16, TN = WTN / 16;
  static constexpr int STAGE = (kBM + BN) * 128;
  static constexpr int CST = BN * 2 + 16;  // C tile row stride: bf16 rows padded 16 B
  // Tile order: the XCD remap gives each XCD a contiguous run of logical tiles (32 at a time on
  // its 32 CUs); logical tiles go through groups of GM m-tiles, M fastest inside a group, so such
  // a run is a GM x (32 / GM) block of tiles that shares GM A panels and 32 / GM B panels in that
  // XCD's L2 — instead of one A panel and 32 B panels (a full row of N tiles), which made every
  // XCD stream all of B (2.6x hipBLASLt's HBM bytes on 8192^3, profiles/r3_pmc_kernels.txt).
  static constexpr int GM = BN == 256 ? 8 : 4;  // 8 x 4 tiles of 256 x 256, 4 x 8 of 256 x 128
  // stages | C tile (+ `extra` bytes an epilogue keeps past the C tile)
  static constexpr size_t lds_bytes(size_t extra = 0) {
    return std::max<size_t>((size_t)2 * STAGE, (size_t)kBM * CST + extra);
  }
};

struct TileOrigin {
  int mt, nt;
};
// block `bid` of a `tiles`-block grid with `ntiles` n-tiles -> its (m-tile, n-tile). Both are
// block-uniform; the divisions leave them in VGPRs, and readfirstlane moves them to SGPRs so the tile
// origin does not hold vector registers across the K loop (the 256 x 256 tile has none to spare).
template <int BN>
__device__ __forceinline__ TileOrigin tile_origin(int bid, int tiles, int ntiles) {
  constexpr int GM = TileGeo<BN>::GM;
  const int wg = dev::xcd_remap(bid, tiles);
  const int mtiles = tiles / ntiles, grp = wg / (GM * ntiles), first_m = grp * GM;
  const int gm = min(mtiles - first_m, GM), local = wg - grp * GM * ntiles;
  return {__builtin_amdgcn_readfirstlane(first_m + local % gm), __builtin_amdgcn_readfirstlane(local / gm)};
}

// LDS-DMA layout: lane l of wave w fills 16-B slot (l & 7) of rows (w + i NW) * 8 + (l >> 3) of
// an operand's stage (wave-instruction i < AI for A, < BI for B); each wave-instruction fills 8
// full 128-B rows. The per-lane SOURCE chunk is pre-swizzled so the lane-linear LDS image has the
// XOR-swizzled chunk order the ds_read_b128 fragment reads want (conflict-free column-slice reads).
__device__ __forceinline__ int dma_row(int lane, int wid) { return wid * 8 + (lane >> 3); }  // + i * 8 NW
// the 16-B source chunk for slot (l & 7) of row `drow`; (row >> 1) & 7 is the same for row + 64 i
__device__ __forceinline__ int dma_src_chunk(int lane, int drow) { return (lane & 7) ^ ((drow >> 1) & 7); }
// The LDS destination of wave-instruction i is byte (wid * 8 + i * 8 NW) * 128 of the operand's
// stage (the lanes follow linearly). The callers spell that one expression out in their `issue`:
// behind a helper it costs the 256 x 256 tile registers (profiles/r9_gemm_pipeline_refactor.txt).

// The K loop. `Ops` are the operand traits:
//   Ops::Frag            one MFMA operand register group
//   Ops::kSteps          MFMAs per (A fragment, B fragment) pair and K-tile; a half's fragments are
//                        Frag[kSteps][H]
//   Ops::pack<H>(f, c)   the H fragments of a half from the 16-B chunks the loop has read: c[kh][i] =
//                        this lane's chunk kh * 4 + (lane >> 4) of fragment i's row
//   Ops::mfma(b, a, c)   one MFMA: B rows as the first operand (the transposed tile, so a lane's
//                        four accumulators are four consecutive output columns of one row)
// `issue(kt, buf)` starts the DMA of K-tile kt into stage buf: exactly AI + BI global_load_lds per
// wave and nothing else that touches vmcnt. `nk` >= 1 K-tiles; acc is accumulated into.
template <int BN, class Ops, class Issue>
__device__ __forceinline__ void k_loop_4phase(int tid, int nk, f32x4 (&acc)[TileGeo<BN>::TM][TileGeo<BN>::TN],
                                              const Issue& issue) {
  // The block's dynamic LDS is named here and the ds_read_b128 below stay in this function's own
  // lambdas, not behind a pointer parameter or in the traits: either indirection changes the register
  // allocation of the 256 x 256 tile at its 256-VGPR ceiling (profiles/r9_gemm_pipeline_refactor.txt).
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  using G = TileGeo<BN>;
  constexpr int AI = G::AI, BI = G::BI, WTM = G::WTM, WTN = G::WTN, TM = G::TM, TN = G::TN, STAGE = G::STAGE;
  constexpr int KS = Ops::kSteps;
  using Frag = typename Ops::Frag;
  const int lane = tid & 63, wid = tid >> 6, wm = wid / kWN, wn = wid % kWN;
  // 4-phase: each K-tile is 4 phases, one per quadrant (A half x B half) of the wave's output,
  // 16 MFMAs each; the fragments of the next phase are read while the current phase's MFMAs
  // run, so the MFMA pipe never waits on LDS. The phase order alternates between even and odd
  // K-tiles so the last phase of a tile and the first of the next use different fragment
  // registers: even (A0,B0) (A0,B1) (A1,B1) (A1,B0), odd (A0,B1) (A0,B0) (A1,B0) (A1,B1).
  // One barrier per K-tile, between phases 1 and 2: by then this wave's reads of the tile's
  // stage are done (lgkmcnt(0)) and its DMA of tile t+1 (issued after the previous tile's
  // barrier, four phases ago) has landed (vmcnt(0) - nothing else is in flight); after it the
  // DMA of tile t+2 goes into this tile's stage and phases 2-3 read the first fragments of t+1.
  constexpr int HA = TM / 2, HB = TN / 2;
  static_assert(HB >= 1, "B halves need at least one 16-column fragment");
  Frag fa0[KS][HA], fa1[KS][HA], fb0[KS][HB], fb1[KS][HB];
  // fragment rows of a wave are row0 + 16 i: the XOR term ((row >> 1) & 7) is the same for all
  // of them, so each 16-B chunk kh needs ONE per-lane byte offset; the rest is an immediate
  const int ra = wm * WTM + (lane & 15), rb = wn * WTN + (lane & 15);
  uint32_t a_lds[2], b_lds[2];
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) {
    a_lds[kh] = ra * 128 + 16 * ((kh * 4 + (lane >> 4)) ^ ((ra >> 1) & 7));
    b_lds[kh] = kBM * 128 + rb * 128 + 16 * ((kh * 4 + (lane >> 4)) ^ ((rb >> 1) & 7));
  }
  auto ldA = [&](Frag (&f)[KS][HA], int half, int buf) {
    u32x4 c[2][HA];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int i = 0; i < HA; ++i)
        c[kh][i] = *reinterpret_cast<const u32x4*>(smem + buf * STAGE + a_lds[kh] + (half * HA + i) * 16 * 128);
    Ops::template pack<HA>(f, c);
  };
  auto ldB = [&](Frag (&f)[KS][HB], int half, int buf) {
    u32x4 c[2][HB];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int j = 0; j < HB; ++j)
        c[kh][j] = *reinterpret_cast<const u32x4*>(smem + buf * STAGE + b_lds[kh] + (half * HB + j) * 16 * 128);
    Ops::template pack<HB>(f, c);
  };
  auto mma = [&](const Frag (&a)[KS][HA], auto ah, const Frag (&b)[KS][HB], auto bh) {
    constexpr int AH = decltype(ah)::value, BHV = decltype(bh)::value;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int i = 0; i < HA; ++i)
#pragma unroll
        for (int j = 0; j < HB; ++j)
          acc[AH * HA + i][BHV * HB + j] = Ops::mfma(b[ks][j], a[ks][i], acc[AH * HA + i][BHV * HB + j]);
  };
  // One phase = the fragment reads for the NEXT phase interleaved into this phase's MFMAs,
  // MFMA first: the wait the compiler puts before the first MFMA then covers only the reads of
  // the previous phase (whose MFMAs hid them), never the ones just issued. sched_barrier(0)
  // keeps every instruction inside its phase.
  auto interleave = [&](auto nld) {
    constexpr int NLD = decltype(nld)::value, NM = KS * HA * HB;
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);       // one MFMA (waits for this phase's fragments)
    __builtin_amdgcn_sched_group_barrier(0x100, NLD, 0);     // the next phase's reads
    __builtin_amdgcn_sched_group_barrier(0x008, NM - 1, 0);  // the rest of the MFMAs
    __builtin_amdgcn_sched_barrier(0);
  };
  using LA = std::integral_constant<int, 2 * HA>;  // reads of an A half (two 16-B chunks per fragment row)
  using LB = std::integral_constant<int, 2 * HB>;
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  // The loop runs tile PAIRS and is branch-free: a wait counter cannot be tracked through a
  // conditional load (the compiler then waits for everything), so the last tiles re-read a
  // valid stage and re-stage the last K-tile instead of skipping; those values are never used.
  // An odd tile count gets a zero tile in front (virtual tile 0 = zeros written to stage 0, real
  // tile k = virtual k + 1): its MFMAs add exact zeros (zero bytes are 0.0 in bf16 and in both FP8
  // formats), and no tail code raises the register pressure of the loop.
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
  issue(1 - odd, 1);  // virtual tile 1: real tile 1 (even count) / 0 (odd count)
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

// The C tile through LDS: fp32 accumulators -> bf16 rows of CST bytes at Cs, 8-B writes (a lane's
// four accumulators are four consecutive columns of one row). `frag(v, col) -> f32x4` is the fp32
// math before the one rounding (col = the first of the four tile columns). The caller has passed
// the barrier after which no wave reads the stages; returns with the tile visible to every wave.
template <int BN, class FragOp>
__device__ __forceinline__ void c_tile_to_lds(uint8_t* Cs, int tid,
                                              const f32x4 (&acc)[TileGeo<BN>::TM][TileGeo<BN>::TN],
                                              const FragOp& frag) {
  using G = TileGeo<BN>;
  const int lane = tid & 63, wid = tid >> 6, wm = wid / kWN, wn = wid % kWN;
#pragma unroll
  for (int i = 0; i < G::TM; ++i)
#pragma unroll
    for (int j = 0; j < G::TN; ++j) {
      const int row = wm * G::WTM + i * 16 + (lane & 15);
      const int col = wn * G::WTN + j * 16 + (lane >> 4) * 4;
      const f32x4 v = frag(acc[i][j], col);
      uint2 pk;
      pk.x = dev::pack_bf16x2(v[0], v[1]);
      pk.y = dev::pack_bf16x2(v[2], v[3]);
      *reinterpret_cast<uint2*>(Cs + row * G::CST + col * 2) = pk;
    }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// The C tile leaves as full 16-B row chunks: thread tid owns chunk column readout_col (= cc, eight
// output columns from cc * 8; the epilogues use the same function for their own addressing) of rows
// tid / CPR + (kThreads / CPR)·i and calls out_row(row, chunk) for those below rows_valid. Each
// batch's LDS reads are issued before its stores (rows past rows_valid read row rows_valid - 1 and
// are skipped): a read-then-use per row compiled to one ds_read + s_waitcnt lgkmcnt(0) round trip
// per row.
template <int BN>
__device__ __forceinline__ int readout_col(int tid) { return tid % (BN / 8); }
template <int BN, class OutRow>
__device__ __forceinline__ void readout_rows(const uint8_t* Cs, int tid, int rows_valid, const OutRow& out_row) {
  constexpr int CST = TileGeo<BN>::CST, CPR = BN / 8;
  static_assert(kThreads % CPR == 0, "readout mapping needs a fixed chunk column per thread");
  constexpr int NIT = kBM * CPR / kThreads, RSTR = kThreads / CPR, EB = NIT < 4 ? NIT : 4;
  static_assert(kBM * CPR % kThreads == 0, "readout rows must divide evenly over the threads");
  const int cc = readout_col<BN>(tid);
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

// a + b over eight packed bf16: fp32 sums, one rounding (the residual epilogues)
__device__ __forceinline__ u32x4 add_bf16x8(u32x4 a, u32x4 b) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
    a[e] = dev::pack_bf16x2(bf(a[e] & 0xffffu) + bf(b[e] & 0xffffu), bf(a[e] >> 16) + bf(b[e] >> 16));
  return a;
}

// ---- host side ----

// Opts kernel Kern in to `lds` bytes of dynamic LDS, once per kernel instantiation.
template <auto Kern>
inline void max_dyn_lds_once(size_t lds) {
  static const bool done = [lds] {
    XDDP_HIP_CHECK(hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return true;
  }();
  (void)done;
}

// Tile width: 256 x 256 unless the 256 x 128 grid fills the CUs' last round better (one block
// per CU: a 256 x 256 grid of 800 tiles on 256 CUs runs 4 rounds, the last 1/8 full).
inline int pick_bn(int64_t M, int64_t N, int cus) {
  if (N % 256) return 128;
  const int64_t mt = (M + kBM - 1) / kBM;
  const int64_t r256 = (mt * (N / 256) + cus - 1) / cus, r128 = (mt * (N / 128) + cus - 1) / cus;
  // a 256 x 128 tile does half the work at ~1.15x the per-FLOP cost (more B traffic per MFMA)
  return 2.0 * r256 <= 1.15 * r128 ? 256 : 128;
}

// Compute units of the device the first call names (cached: one device model per process); 256,
// the MI355X count, if the query fails.
inline int cu_count(int device_index) {
  static const int cached = [&] {
    int v = 0;
    return hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device_index) == hipSuccess && v > 0 ? v : 256;
  }();
  return cached;
}

}  // namespace kernels
}  // namespace xddp
