// Window attention with an additive relative-position bias and a label mask (Swin and its kin) for
// gfx950 MFMA: bf16, head width 32, windows of 1 <= N <= 64 tokens (7 x 7 = 49 for Swin).
//
// qkv is the QKV projection's output viewed [Bw, N, 3, H, 32]; o is [Bw, N, H, 32], ready for the
// output projection; dqkv has qkv's layout, ready for the projection's backward. bias is [H, N, N]
// (bf16 or fp32), labels [nW, N] int32: window w uses row w % nW, and query i sees key j iff their
// labels are equal (Swin's shifted-window 0 / -100 table has this structure). Masked and padded keys
// get weight exactly 0.
//
// One wave owns one (window, head) at a time; N is padded to 64 in LDS only (rows N..63 are written
// as zeros, so no padding value ever reaches an MFMA). A workgroup is NW waves that share one head
// and walk a chunk of windows (window c0 + wave, + NW, ...): grid = (chunks, heads). Each wave
// fetches the head's bias once, into registers in the accumulator layout, already times log2 e and
// with the key padding folded in as a large negative constant. The next window's q, k, v (and dO)
// rows are loaded into registers (16 B per lane and load) while the current window is computed (in
// the backward: from its dS on, where the registers are free) and written to LDS after it; only the
// wave itself reads its tiles, so the window loop has no barrier.
//
// Tiles are row-major [64][32] bf16 with a 16-B chunk XOR swizzle that is conflict-free both for
// ds_read_b128 row fragments and for ds_read_b64_tr_b16 transposed fragments, so a tile is staged
// once whichever way it is read.
//
// Forward, 16 MFMAs (mfma_f32_32x32x16_bf16) per (window, head):
// * S^T = K·Q^T, 2 x 2 tiles x 2 k-steps, K as the A operand and Q^T as the B operand, so a lane
//   owns one query row of each query tile and half of the keys: row max and sum are in-lane plus
//   one exchange with lane ^ 32. The whole row is there, so the softmax is one pass;
// * exp2-domain softmax: s = acc · (scale·log2 e) + bias·log2 e in fp32 after the MFMA;
// * O^T = V^T·P^T: V^T by the transposing LDS read, P^T is the score accumulator rounded to bf16
//   once (the accumulator layout is the B-operand layout when V's rows are read in kappa order).
//
// Backward, one kernel, 40 MFMAs: S^T and dP^T = V·dO^T (query on the lane), P and
// dS = P∘(dP − δ), δ = rowsum(P∘dP), in fp32 in registers; nothing but qkv, bias and labels is
// saved by the forward. dQ^T = K^T·dS^T takes dS straight from the registers (key reduction). dV^T =
// dO^T·P and dK^T = Q^T·dS reduce over the query: P and dS (bf16, rounded once) go through one
// [64][64] LDS tile, written by rows and read back with the transposing read. Rows and columns of P
// and dS at or past N and masked entries are exactly zero. dbias: each wave accumulates dS (fp32,
// before rounding) over its windows in registers, the workgroup's waves are summed in wave order
// through LDS, one [H, N, N] fp32 partial per chunk is written, and a second kernel sums the chunks
// in index order. No atomics; the chunking depends on Bw and H only, so results are repeatable and
// equal on every replica. LDS: forward 4 x 12.25 KB, backward 2 x 24.25 KB per workgroup.
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include "common.h"
#include "kernels/dev_utils.h"
#include "kernels/norm.h"

namespace xddp {
namespace kernels {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short v4s __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
using dev::u32x4;

constexpr int kD = 32;           // head width
constexpr int kT = 64;           // padded window length
constexpr int kTile = kT * kD * 2;  // bytes of one [64][32] bf16 tile
constexpr int kPS = kT * kT * 2;    // bytes of the [64][64] bf16 P / dS tile
constexpr float kNeg = -1e30f;      // masked / padded score (log2 domain); anything below kNeg / 2 gets weight 0
constexpr float kLog2e = 1.44269504088896341f;
constexpr int kFwdWaves = 4, kBwdWaves = 2;
constexpr int kTargetGroups = 1024;  // workgroups aimed at when the windows are cut into chunks

__device__ __forceinline__ v4s lds_tr16(const uint8_t* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(p));
}
__device__ __forceinline__ f32x16 mfma32(const bf16x8& a, const bf16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// the wave's LDS writes have landed before its reads that follow (one wave per tile: no barrier)
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// 16-B chunk swizzle of a row-major [rows][W] bf16 tile. W = 32 (4 chunks per row): 16 consecutive
// rows at one chunk (b128 row fragments) cover 4 row phases x 4 swizzled chunks = all 64 banks once;
// the 4 consecutive rows x 4 chunks of a transposed read share one row >> 2 and stay distinct.
// W = 64 (8 chunks): the flash kernels' D = 64 form.
template <int W>
__device__ __forceinline__ int uswz(int row, int chunk) {
  return chunk ^ (W == 32 ? ((row >> 2) & 3) : (4 * ((row >> 1) & 1) | ((row >> 2) & 3)));
}

// rows held by lane group g (= lane >> 5) in element e (0..7) of a 16-wide k-step of a 32x32
// accumulator; element i (0..15) of the accumulator is row kappa(g, i & 7) + 16 (i >> 3)
__device__ __forceinline__ int kappa(int g, int e) { return 4 * g + (e & 3) + 8 * (e >> 2); }

// row fragment of a [64][32] tile: row r, 8 elements from column 16 ks + 8 (lane >> 5)
__device__ __forceinline__ bf16x8 ld_rowfrag(const uint8_t* T, int r, int ks, int lane) {
  return *reinterpret_cast<const bf16x8*>(T + r * (kD * 2) + uswz<kD>(r, 2 * ks + (lane >> 5)) * 16);
}

// transposed fragment of a [64][W] tile: element e of lane l = T[rbase + kappa(g, e)][cbase + (l & 31)]
template <int W>
__device__ __forceinline__ bf16x8 ld_trfrag(const uint8_t* T, int rbase, int cbase, int lane) {
  const int g = lane >> 5, q4 = (lane & 15) >> 2, p4 = lane & 3;
  const int col = cbase + 16 * ((lane >> 4) & 1) + 4 * p4;  // 4 bf16 = 8 B per lane
  const int r0 = rbase + 4 * g + q4, r1 = r0 + 8;
  const int c0 = col >> 3, off = (col & 7) * 2;
  const v4s lo = lds_tr16(T + r0 * (W * 2) + uswz<W>(r0, c0) * 16 + off);
  const v4s hi = lds_tr16(T + r1 * (W * 2) + uswz<W>(r1, c0) * 16 + off);
  const v4s v8[2] = {lo, hi};
  return __builtin_bit_cast(bf16x8, v8);
}

// One wave's register-staged [64][32] tile: lane l holds the 16-B chunks q = l + 64 j (row q / 4,
// chunk q % 4); rows at or past n are zeros.
struct TileRegs {
  u32x4 v[4];
  __device__ __forceinline__ void load(const uint16_t* base, int64_t row_stride, int n, int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = lane + 64 * j, r = q >> 2, c = q & 3;
      v[j] = r < n ? *reinterpret_cast<const u32x4*>(base + r * row_stride + c * 8) : u32x4{0, 0, 0, 0};
    }
  }
  __device__ __forceinline__ void store(uint8_t* T, int lane) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = lane + 64 * j, r = q >> 2, c = q & 3;
      *reinterpret_cast<u32x4*>(T + r * (kD * 2) + uswz<kD>(r, c) * 16) = v[j];
    }
  }
};

// The head's bias in the accumulator layout, times log2 e: b[u][t][i] belongs to query 32 u +
// (lane & 31) and key 32 t + kappa(..). Keys at or past n carry kNeg, padded queries 0.
// kind: 0 none, 1 bf16, 2 fp32.
__device__ __forceinline__ void load_bias(f32x16 (&b)[2][2], const void* bias, int kind, int h, int n, int lane) {
  const int g = lane >> 5;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int q = 32 * u + (lane & 31);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = 32 * t + kappa(g, i & 7) + 16 * (i >> 3);
        float x = 0.f;
        if (q < n && k < n && kind != 0) {
          const int64_t at = ((int64_t)h * n + q) * n + k;
          x = kind == 1 ? dev::bf16_to_f32(reinterpret_cast<const uint16_t*>(bias)[at])
                        : reinterpret_cast<const float*>(bias)[at];
        }
        b[u][t][i] = k < n ? x * kLog2e : kNeg;
      }
  }
}

__device__ __forceinline__ void zero(f32x16 (&a)[2][2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) a[u][t][i] = 0.f;
}

// sc[u][t] = (A tile rows 32 t..)(B tile rows 32 u..)^T over the 32 columns: [A row][B row on the lane]
__device__ __forceinline__ void rows_times_rows(f32x16 (&sc)[2][2], const uint8_t* A, const uint8_t* B, int lane) {
  zero(sc);
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    bf16x8 a[2], b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) a[t] = ld_rowfrag(A, 32 * t + (lane & 31), ks, lane);
#pragma unroll
    for (int u = 0; u < 2; ++u) b[u] = ld_rowfrag(B, 32 * u + (lane & 31), ks, lane);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int t = 0; t < 2; ++t) sc[u][t] = mfma32(a[t], b[u], sc[u][t]);
  }
}

// In place: raw scores S^T -> P^T (fp32, rows sum to 1). labs: the window's 64 labels in LDS.
// Masked keys, padded keys and (every entry of) padded query rows come out exactly 0.
template <bool LAB>
__device__ __forceinline__ void softmax_rows(f32x16 (&sc)[2][2], const f32x16 (&b)[2][2], const int* labs,
                                             float scale_log2, int n, int lane) {
  const int g = lane >> 5;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int q = 32 * u + (lane & 31);
    int lq = 0;
    if constexpr (LAB) lq = labs[q];
    float mx = kNeg;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        i32x4 lk = {0, 0, 0, 0};
        if constexpr (LAB) lk = *reinterpret_cast<const i32x4*>(labs + 32 * t + 4 * g + 8 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float s = fmaf(sc[u][t][4 * j + e], scale_log2, b[u][t][4 * j + e]);
          if (LAB && lk[e] != lq) s = kNeg;
          sc[u][t][4 * j + e] = s;
          mx = fmaxf(mx, s);
        }
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float s = sc[u][t][i];
        const float p = s > 0.5f * kNeg ? __builtin_amdgcn_exp2f(s - mx) : 0.f;
        sc[u][t][i] = p;
        l += p;
      }
    l += __shfl_xor(l, 32, 64);
    const float inv = (q < n && l > 0.f) ? 1.f / l : 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) sc[u][t][i] *= inv;
  }
}

// fp32 accumulator tiles [key][query on the lane] -> bf16 B operands of the four 16-key steps
__device__ __forceinline__ void to_bf16(bf16x8 (&f)[2][4], const f32x16 (&a)[2][2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      uint32_t pk[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        pk[e] = dev::pack_bf16x2(a[u][kk >> 1][8 * (kk & 1) + 2 * e], a[u][kk >> 1][8 * (kk & 1) + 2 * e + 1]);
      f[u][kk] = __builtin_bit_cast(bf16x8, pk);
    }
}

// out^T[u] = T^T·f[u]: [column of T][query on the lane], the reduction walking T's 64 rows (keys)
__device__ __forceinline__ void cols_times_frags(f32x16 (&out)[2], const uint8_t* T, const bf16x8 (&f)[2][4], int lane) {
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int i = 0; i < 16; ++i) out[u][i] = 0.f;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const bf16x8 a = ld_trfrag<kD>(T, 16 * kk, 0, lane);
#pragma unroll
    for (int u = 0; u < 2; ++u) out[u] = mfma32(a, f[u][kk], out[u]);
  }
}

// bf16 fragments f (rows = queries on the lane, elements = keys) -> the [query][key] tile PS
__device__ __forceinline__ void store_ps(uint8_t* PS, const bf16x8 (&f)[2][4], int lane) {
  const int g = lane >> 5;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int q = 32 * u + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const u32x4 w = __builtin_bit_cast(u32x4, f[u][kk]);
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {  // keys 16 kk + 8 jj + 4 g + 0..3: chunk 2 kk + jj, 8 B at byte 8 g
        uint2 v;
        v.x = w[2 * jj];
        v.y = w[2 * jj + 1];
        *reinterpret_cast<uint2*>(PS + q * (kT * 2) + uswz<kT>(q, 2 * kk + jj) * 16 + 8 * g) = v;
      }
    }
  }
}

// out^T[t] = T^T·PS[:, 32 t..]: [column of T][key 32 t + (lane & 31)], the reduction walking the 64 queries
__device__ __forceinline__ void cols_times_ps(f32x16 (&out)[2], const uint8_t* T, const uint8_t* PS, int lane) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) out[t][i] = 0.f;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const bf16x8 a = ld_trfrag<kD>(T, 16 * kk, 0, lane);
#pragma unroll
    for (int t = 0; t < 2; ++t) out[t] = mfma32(a, ld_trfrag<kT>(PS, 16 * kk, 32 * t, lane), out[t]);
  }
}

// acc[u][i] = value (times mul) for row 32 u + (lane & 31), column kappa(..) -> 32-wide bf16 rows of dst
__device__ __forceinline__ void store_rows(uint16_t* dst, int64_t row_stride, const f32x16 (&acc)[2], float mul, int n,
                                           int lane) {
  const int g = lane >> 5;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int r = 32 * u + (lane & 31);
    if (r < n) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // 4 consecutive columns per store: 4 g + 8 j + 0..3
        uint2 pk;
        pk.x = dev::pack_bf16x2(acc[u][4 * j] * mul, acc[u][4 * j + 1] * mul);
        pk.y = dev::pack_bf16x2(acc[u][4 * j + 2] * mul, acc[u][4 * j + 3] * mul);
        *reinterpret_cast<uint2*>(dst + r * row_stride + 4 * g + 8 * j) = pk;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ fwd
// Without labels the kernel fits 256 registers, so two workgroups share a CU (two waves per SIMD); the
// label form would spill three registers at that limit and keeps one.
template <int NW, bool LAB>
__global__ __launch_bounds__(64 * NW, LAB ? 1 : 2) void wa_fwd_kernel(const uint16_t* __restrict__ qkv, const void* __restrict__ bias,
                                                         int bias_kind, const int* __restrict__ labels, int nW,
                                                         uint16_t* __restrict__ O, int Bw, int N, int H, int cw,
                                                         float scale_log2) {
  __shared__ __attribute__((aligned(16))) uint8_t tiles[NW][3][kTile];
  __shared__ __attribute__((aligned(16))) int labs_all[NW][kT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = blockIdx.y;
  uint8_t* Qt = tiles[wave][0];
  uint8_t* Kt = tiles[wave][1];
  uint8_t* Vt = tiles[wave][2];
  int* labs = labs_all[wave];
  const int64_t rs = (int64_t)3 * H * kD, ws = (int64_t)N * rs;  // row and window strides of qkv
  const int wend = min(Bw, ((int)blockIdx.x + 1) * cw);
  int w = (int)blockIdx.x * cw + wave;
  if (w >= wend) return;
  f32x16 b[2][2];
  load_bias(b, bias, bias_kind, h, N, lane);
  TileRegs rq, rk, rv;
  int rl = 0;
  auto fetch = [&](int win) {
    const uint16_t* base = qkv + win * ws + h * kD;
    rq.load(base, rs, N, lane);
    rk.load(base + H * kD, rs, N, lane);
    rv.load(base + 2 * H * kD, rs, N, lane);
    if constexpr (LAB) rl = lane < N ? labels[(int64_t)(win % nW) * N + lane] : 0;
  };
  fetch(w);
  for (; w < wend; w += NW) {
    rq.store(Qt, lane);
    rk.store(Kt, lane);
    rv.store(Vt, lane);
    if constexpr (LAB) labs[lane] = rl;
    wave_lds_sync();
    if (w + NW < wend) fetch(w + NW);  // in flight during this window's math
    f32x16 sc[2][2];
    rows_times_rows(sc, Kt, Qt, lane);
    softmax_rows<LAB>(sc, b, labs, scale_log2, N, lane);
    bf16x8 pf[2][4];
    to_bf16(pf, sc);
    f32x16 o[2];
    cols_times_frags(o, Vt, pf, lane);
    store_rows(O + ((int64_t)w * N * H + h) * kD, (int64_t)H * kD, o, 1.f, N, lane);
    wave_lds_sync();  // the reads are done before the next window overwrites the tiles
  }
}

// ------------------------------------------------------------------------------------------ bwd
template <int NW, bool LAB, bool DB>
__global__ __launch_bounds__(64 * NW) void wa_bwd_kernel(const uint16_t* __restrict__ qkv, const void* __restrict__ bias,
                                                         int bias_kind, const int* __restrict__ labels, int nW,
                                                         const uint16_t* __restrict__ dO, uint16_t* __restrict__ dqkv,
                                                         float* __restrict__ partials, int Bw, int N, int H, int cw,
                                                         float scale_log2, float scale) {
  __shared__ __attribute__((aligned(16))) uint8_t tiles[NW][4][kTile];  // Q, K, V, dO; then a wave's dbias sum
  __shared__ __attribute__((aligned(16))) uint8_t ps_all[NW][kPS];
  __shared__ __attribute__((aligned(16))) int labs_all[NW][kT];
  static_assert(4 * kTile == 4 * 16 * 64 * (int)sizeof(float), "a wave's four tiles hold its dbias accumulators");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = blockIdx.y, g = lane >> 5;
  uint8_t* Qt = tiles[wave][0];
  uint8_t* Kt = tiles[wave][1];
  uint8_t* Vt = tiles[wave][2];
  uint8_t* Gt = tiles[wave][3];
  uint8_t* PS = ps_all[wave];
  int* labs = labs_all[wave];
  const int64_t rs = (int64_t)3 * H * kD, ws = (int64_t)N * rs;
  const int wend = min(Bw, ((int)blockIdx.x + 1) * cw);
  int w = (int)blockIdx.x * cw + wave;
  f32x16 db[2][2];
  if constexpr (DB) zero(db);
  if (w < wend) {
    f32x16 b[2][2];
    load_bias(b, bias, bias_kind, h, N, lane);
    TileRegs rq, rk, rv, rg;
    int rl = 0;
    auto fetch = [&](int win) {
      const uint16_t* base = qkv + win * ws + h * kD;
      rq.load(base, rs, N, lane);
      rk.load(base + H * kD, rs, N, lane);
      rv.load(base + 2 * H * kD, rs, N, lane);
      rg.load(dO + ((int64_t)win * N * H + h) * kD, (int64_t)H * kD, N, lane);
      if constexpr (LAB) rl = lane < N ? labels[(int64_t)(win % nW) * N + lane] : 0;
    };
    fetch(w);
    for (; w < wend; w += NW) {
      rq.store(Qt, lane);
      rk.store(Kt, lane);
      rv.store(Vt, lane);
      rg.store(Gt, lane);
      if constexpr (LAB) labs[lane] = rl;
      wave_lds_sync();
      f32x16 p[2][2], ds[2][2];
      rows_times_rows(p, Kt, Qt, lane);
      softmax_rows<LAB>(p, b, labs, scale_log2, N, lane);
      rows_times_rows(ds, Vt, Gt, lane);  // dP^T = V·dO^T
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float delta = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int i = 0; i < 16; ++i) delta = fmaf(p[u][t][i], ds[u][t][i], delta);
        delta += __shfl_xor(delta, 32, 64);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            ds[u][t][i] = p[u][t][i] * (ds[u][t][i] - delta);  // P = 0 exactly where masked or padded
            if constexpr (DB) db[u][t][i] += ds[u][t][i];
          }
      }
      // the next window's rows are in flight during the 24 MFMAs below and their stores (issued here,
      // not before S and dP: the staging registers on top of p, dP, bias and dbias would spill)
      if (w + NW < wend) fetch(w + NW);
      bf16x8 f[2][4];
      f32x16 acc[2];
      uint16_t* dst = dqkv + w * ws + h * kD;
      to_bf16(f, p);
      store_ps(PS, f, lane);
      wave_lds_sync();
      cols_times_ps(acc, Gt, PS, lane);  // dV^T = dO^T·P
      store_rows(dst + 2 * H * kD, rs, acc, 1.f, N, lane);
      to_bf16(f, ds);
      wave_lds_sync();  // dV's reads of P are done
      store_ps(PS, f, lane);
      cols_times_frags(acc, Kt, f, lane);  // dQ^T = K^T·dS^T
      store_rows(dst, rs, acc, scale, N, lane);
      wave_lds_sync();
      cols_times_ps(acc, Qt, PS, lane);  // dK^T = Q^T·dS
      store_rows(dst + H * kD, rs, acc, scale, N, lane);
      wave_lds_sync();
    }
  }
  if constexpr (DB) {
    // the waves' sums in wave order: wave 0 + wave 1 + ..., then one [N][N] partial of this (chunk, head)
    float* mine = reinterpret_cast<float*>(tiles[wave][0]);
    if (wave > 0) {
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int i = 0; i < 16; ++i) mine[((2 * u + t) * 16 + i) * 64 + lane] = db[u][t][i];
    }
    __syncthreads();
    if (wave == 0) {
      float* out = partials + ((int64_t)blockIdx.x * H + h) * N * N;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int q = 32 * u + (lane & 31);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            float s = db[u][t][i];
            for (int v = 1; v < NW; ++v)
              s += reinterpret_cast<const float*>(tiles[v][0])[((2 * u + t) * 16 + i) * 64 + lane];
            const int k = 32 * t + kappa(g, i & 7) + 16 * (i >> 3);
            if (q < N && k < N) out[q * N + k] = s;
          }
      }
    }
  }
}

// dbias[e] = sum over the chunks, in index order, of partials[chunk][e]; OutT float or bf16 bits
template <typename OutT>
__global__ __launch_bounds__(256) void wa_dbias_reduce_kernel(const float* __restrict__ partials, OutT* __restrict__ out,
                                                              int nchunks, int64_t elems) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= elems) return;
  float s = 0.f;
  for (int c = 0; c < nchunks; ++c) s += partials[c * elems + e];
  if constexpr (sizeof(OutT) == 4) out[e] = s;
  else out[e] = dev::f32_to_bf16(s);
}

struct Problem {
  int Bw, N, H, nW, bias_kind;
  const void* bias;
  const int* labels;
};

Problem check_problem(const char* who, const at::Tensor& qkv, const c10::optional<at::Tensor>& bias,
                      const c10::optional<at::Tensor>& labels) {
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 && qkv.dim() == 5 && qkv.size(2) == 3 &&
                  qkv.size(4) == kD && qkv.is_contiguous() && reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0,
              who, ": qkv must be a dense, 16-byte aligned bf16 [Bw, N, 3, H, 32] tensor on the GPU");
  Problem p{};
  p.Bw = (int)qkv.size(0), p.N = (int)qkv.size(1), p.H = (int)qkv.size(3);
  TORCH_CHECK(qkv.size(0) < (1 << 30) && p.N >= 1 && p.N <= kT && p.H >= 1 && p.H < 65536, who,
              ": 1 <= N <= 64 and H < 65536");
  if (bias.has_value()) {
    TORCH_CHECK(bias->device() == qkv.device() && bias->is_contiguous() && bias->dim() == 3 && bias->size(0) == p.H &&
                    bias->size(1) == p.N && bias->size(2) == p.N &&
                    (bias->scalar_type() == at::kBFloat16 || bias->scalar_type() == at::kFloat),
                who, ": bias must be a contiguous bf16 or fp32 [H, N, N] tensor on qkv's device");
    p.bias_kind = bias->scalar_type() == at::kBFloat16 ? 1 : 2;
    p.bias = bias->data_ptr();
  }
  if (labels.has_value()) {
    TORCH_CHECK(labels->device() == qkv.device() && labels->is_contiguous() && labels->dim() == 2 &&
                    labels->size(1) == p.N && labels->scalar_type() == at::kInt && labels->size(0) >= 1 &&
                    p.Bw % labels->size(0) == 0,
                who, ": labels must be a contiguous int32 [nW, N] tensor on qkv's device with Bw % nW == 0");
    p.nW = (int)labels->size(0);
    p.labels = labels->data_ptr<int>();
  }
  return p;
}

// windows per chunk: a multiple of the waves per workgroup, from Bw and H alone
int chunk_windows(int Bw, int H, int nw) {
  const int64_t per = ((int64_t)Bw * H + kTargetGroups - 1) / kTargetGroups;
  return (int)std::max<int64_t>(2 * nw, (per + nw - 1) / nw * nw);
}

}  // namespace

at::Tensor window_attn_forward(const at::Tensor& qkv, const c10::optional<at::Tensor>& bias,
                               const c10::optional<at::Tensor>& labels, double scale) {
  const Problem p = check_problem("window_attn_forward", qkv, bias, labels);
  auto o = at::empty({p.Bw, p.N, p.H, kD}, qkv.options());
  if (p.Bw == 0) return o;
  auto stream = c10::hip::getCurrentHIPStream(qkv.device().index()).stream();
  const int cw = chunk_windows(p.Bw, p.H, kFwdWaves);
  const dim3 grid((p.Bw + cw - 1) / cw, p.H);
  const auto* q = reinterpret_cast<const uint16_t*>(qkv.data_ptr());
  auto* op = reinterpret_cast<uint16_t*>(o.data_ptr());
  const float sl2 = (float)(scale * 1.4426950408889634);
  if (p.labels)
    wa_fwd_kernel<kFwdWaves, true><<<grid, 64 * kFwdWaves, 0, stream>>>(q, p.bias, p.bias_kind, p.labels, p.nW, op, p.Bw,
                                                                       p.N, p.H, cw, sl2);
  else
    wa_fwd_kernel<kFwdWaves, false><<<grid, 64 * kFwdWaves, 0, stream>>>(q, p.bias, p.bias_kind, nullptr, 1, op, p.Bw,
                                                                        p.N, p.H, cw, sl2);
  XDDP_HIP_CHECK(hipGetLastError());
  return o;
}

std::vector<at::Tensor> window_attn_backward(const at::Tensor& qkv, const c10::optional<at::Tensor>& bias,
                                             const c10::optional<at::Tensor>& labels, const at::Tensor& d_out,
                                             double scale, bool need_dbias) {
  const Problem p = check_problem("window_attn_backward", qkv, bias, labels);
  TORCH_CHECK(d_out.device() == qkv.device() && d_out.scalar_type() == at::kBFloat16 && d_out.is_contiguous() &&
                  d_out.dim() == 4 && d_out.size(0) == p.Bw && d_out.size(1) == p.N && d_out.size(2) == p.H &&
                  d_out.size(3) == kD && reinterpret_cast<uintptr_t>(d_out.data_ptr()) % 16 == 0,
              "window_attn_backward: d_out must be a dense, 16-byte aligned bf16 [Bw, N, H, 32] tensor on qkv's device");
  TORCH_CHECK(!need_dbias || p.bias_kind != 0, "window_attn_backward: need_dbias without a bias");
  auto dqkv = at::empty_like(qkv);
  at::Tensor dbias;
  if (need_dbias) dbias = at::empty_like(*bias);
  if (p.Bw == 0) {
    if (need_dbias) dbias.zero_();
    return {dqkv, dbias};
  }
  auto stream = c10::hip::getCurrentHIPStream(qkv.device().index()).stream();
  const int cw = chunk_windows(p.Bw, p.H, kBwdWaves);
  const int nchunks = (p.Bw + cw - 1) / cw;
  const dim3 grid(nchunks, p.H);
  at::Tensor partials;
  if (need_dbias) partials = at::empty({nchunks, p.H, p.N, p.N}, qkv.options().dtype(at::kFloat));
  const auto* q = reinterpret_cast<const uint16_t*>(qkv.data_ptr());
  const auto* g = reinterpret_cast<const uint16_t*>(d_out.data_ptr());
  auto* dq = reinterpret_cast<uint16_t*>(dqkv.data_ptr());
  float* pp = need_dbias ? partials.data_ptr<float>() : nullptr;
  const float sl2 = (float)(scale * 1.4426950408889634), sc = (float)scale;
  const int nW = p.labels ? p.nW : 1;
#define XDDP_WA_BWD(LAB, DB)                                                                                        \
  wa_bwd_kernel<kBwdWaves, LAB, DB><<<grid, 64 * kBwdWaves, 0, stream>>>(q, p.bias, p.bias_kind, p.labels, nW, g, dq, \
                                                                         pp, p.Bw, p.N, p.H, cw, sl2, sc)
  if (p.labels && need_dbias) XDDP_WA_BWD(true, true);
  else if (p.labels) XDDP_WA_BWD(true, false);
  else if (need_dbias) XDDP_WA_BWD(false, true);
  else XDDP_WA_BWD(false, false);
#undef XDDP_WA_BWD
  XDDP_HIP_CHECK(hipGetLastError());
  if (need_dbias) {
    const int64_t elems = (int64_t)p.H * p.N * p.N;
    const int blocks = (int)((elems + 255) / 256);
    if (p.bias_kind == 2)
      wa_dbias_reduce_kernel<float><<<blocks, 256, 0, stream>>>(pp, dbias.data_ptr<float>(), nchunks, elems);
    else
      wa_dbias_reduce_kernel<uint16_t><<<blocks, 256, 0, stream>>>(pp, reinterpret_cast<uint16_t*>(dbias.data_ptr()),
                                                                   nchunks, elems);
    XDDP_HIP_CHECK(hipGetLastError());
  }
  return {dqkv, dbias};
}

}  // namespace kernels
}  // namespace xddp
