// Fused Adafactor (Shazeer & Stern 2018; torch.optim.Adafactor semantics) for gfx950.
//
// Adafactor keeps, per weight matrix, one row vector and one column vector of second moments. The
// update of an element needs the row sums and the column sums of g'^2 over the whole matrix, and
// the RMS of the whole update before any of it is applied, so this is not a flat element stream:
// parameters of dim >= 2 are walked as [B, R, C] planes in kTR x kTC tiles, described by a 2-D
// segment table passed by value. A step is five stream-ordered launches per table of 40 tensors:
//
//   1. af_stats_kernel   one block per tile: reads g and w once. A thread owns 8 columns of
//                        kTR / 8 rows; column sums of g'^2 stay in registers over the rows and are
//                        folded across the 8 row groups through LDS, row sums are folded across the
//                        32 lanes of a row with __shfl_xor. Writes colp[b][row tile][C],
//                        rowp[b][R][column tile] and one sum(w^2) per tile, each to its own slot.
//   2. af_fold_kernel    per matrix one block per 2048 rows that sums each row's partials in
//                        column-tile order, updates row_var and writes the sum of the new row_var
//                        to rvp[b][block], and one block per 256 columns that sums the column
//                        partials in row-tile order and updates col_var.
//   3. af_usq_kernel     one block per tile: reads g and the factors, writes sum(u^2) per tile.
//                        (Every tile block of passes 3 and 5 adds the matrix's rvp in block order
//                        for max(mean row_var, eps1): at most 63 values for 128256 rows.)
//   4. af_coef_kernel    one block per tensor folds sum(w^2) and sum(u^2) over its tiles:
//                        max(eps2, RMS(w)) rho / max(1, RMS(u) / d).
//   5. af_apply_kernel   one block per tile: reads g, w and the factors, writes w (and with
//                        masters the rounded parameter).
//
// Parameters of dim <= 1 take the three-stage flat pattern of LAMB (multi_tensor.hip) on 8192-element
// chunks. Every partial has a fixed slot and every fold a fixed order; there are no float atomics,
// no host synchronisation, and the only scratch is the partial slabs. A tensor's partials depend on
// that tensor alone, so its result is bitwise the same alone, in any list, and on every replica.
#include "kernels/multi_tensor.h"

#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "common.h"
#include "kernels/dev_utils.h"
#include "kernels/mt_common.h"

namespace xddp {
namespace kernels {

constexpr int kTR = 64, kTC = 256;               // the tile: rows x columns
constexpr int kLanesC = kTC / 8;                 // lanes across a tile row, 8 columns each
constexpr int kRowGroups = kThreads / kLanesC;   // rows in flight per iteration
constexpr int kRowIters = kTR / kRowGroups;      // rows per thread
constexpr int kFoldCols = kThreads;              // columns per column-fold block
constexpr int kFoldRows = kThreads * 8;          // rows per row-fold block
static_assert(kLanesC == 32 && kTR % kRowGroups == 0, "a tile row is one half of a 64-lane wave");

// Slots {w (fp32 master, or the parameter), grad, row_var, col_var, this tensor's scratch, the
// model's parameter (masters only)}. Tiles and fold blocks are numbered over the table.
struct MatTable {
  void* ptr[6][kMaxSeg];
  int32_t B[kMaxSeg], R[kMaxSeg], C[kMaxSeg];
  int32_t tile_end[kMaxSeg];  // inclusive prefix sums of blocks per segment
  int32_t fold_end[kMaxSeg];
  uint64_t vec;  // bit s: every base of segment s is 16-byte aligned and C % 8 == 0
  int32_t nseg;
};
static_assert(kMaxSeg <= 64, "one bit per segment");
static_assert(sizeof(MatTable) + 128 <= 4096, "the by-value segment table must fit the kernarg segment");

struct AfArgs {
  float omb, rho, eps1, e2, eps2, d, decay;  // e2 = eps1^2, decay = 1 - lr * weight_decay
  bool maximize;
  const float* gs;
};

// Geometry and scratch layout of one [B, R, C] tensor
struct Mat {
  int B, R, C, nRT, nCT, nCB, nRB;
  int64_t tiles, o_rowp, o_wsq, o_usq, o_rvp, o_coef;  // offsets in floats from the scratch base
  float* base;
  __host__ __device__ Mat(float* scratch, int B_, int R_, int C_)
      : B(B_), R(R_), C(C_), nRT((R_ + kTR - 1) / kTR), nCT((C_ + kTC - 1) / kTC),
        nCB((C_ + kFoldCols - 1) / kFoldCols), nRB((R_ + kFoldRows - 1) / kFoldRows), base(scratch) {
    tiles = (int64_t)B * nRT * nCT;
    o_rowp = (int64_t)B * nRT * C;
    o_wsq = o_rowp + (int64_t)B * R * nCT;
    o_usq = o_wsq + tiles;
    o_rvp = o_usq + tiles;
    o_coef = o_rvp + (int64_t)B * nRB;
  }
  __host__ __device__ int64_t scratch_floats() const { return o_coef + 1; }
  __host__ __device__ int64_t fold_blocks() const { return (int64_t)B * (nRB + nCB); }
  __device__ float* colp() const { return base; }           // [B][nRT][C]  column sums of a row tile
  __device__ float* rowp() const { return base + o_rowp; }  // [B][R][nCT]  row sums of a column tile
  __device__ float* wsq() const { return base + o_wsq; }    // [tiles]      sum(w^2)
  __device__ float* usq() const { return base + o_usq; }    // [tiles]      sum(u^2)
  __device__ float* rvp() const { return base + o_rvp; }    // [B][nRB]     sums of the new row_var per fold block
  __device__ float* coef() const { return base + o_coef; }  // alpha / max(1, RMS(u) / d)
};

__device__ __forceinline__ int find_end(const int32_t (&end)[kMaxSeg], int nseg, int b) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (b < end[mid]) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The tile of a block: segment s, matrix b, row tile rt, column tile ct, tile index tl in the tensor
struct Tile {
  int s, b, rt, ct;
  int64_t tl;
};
__device__ __forceinline__ Tile block_tile(const MatTable& t) {
  const int s = find_end(t.tile_end, t.nseg, blockIdx.x);
  const int tl = blockIdx.x - (s ? t.tile_end[s - 1] : 0);
  const int nCT = (t.C[s] + kTC - 1) / kTC, per = ((t.R[s] + kTR - 1) / kTR) * nCT;
  return {s, tl / per, (tl % per) / nCT, tl % nCT, tl};
}

// 8 consecutive elements of row `row` from column `col0`; 0 outside the matrix
template <typename T>
__device__ __forceinline__ void ld_row8(const T* base, int row, int col0, int R, int C, bool vec, float (&v)[8]) {
  if (vec && row < R && col0 + 8 <= C) {
    Vec8<T>::ld(base + (int64_t)row * C + col0, v);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      v[j] = (row < R && col0 + j < C) ? Elem<T, float>::ld(base, (int64_t)row * C + col0 + j) : 0.f;
  }
}
template <typename T>
__device__ __forceinline__ void st_row8(T* base, int row, int col0, int R, int C, bool vec, const float (&v)[8]) {
  if (vec && row < R && col0 + 8 <= C) {
    Vec8<T>::st(base + (int64_t)row * C + col0, v);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (row < R && col0 + j < C) Elem<T, float>::st(base, (int64_t)row * C + col0 + j, v[j]);
  }
}

// torch's lerp: the form that is exact at weight 1 (the first step: omb = 1)
__device__ __forceinline__ float af_lerp(float a, float b, float w) {
  const float diff = b - a;
  return w < 0.5f ? fmaf(w, diff, a) : fmaf(-(1.f - w), diff, b);
}
// clamp(min) that keeps NaN, as torch's does
__device__ __forceinline__ float af_floor(float x, float lo) { return x < lo ? lo : x; }

// The update direction u = g' rsqrt(max(rf cf, eps1^2)), rf = row_var / max(mean row_var, eps1) and
// cf = col_var (1-D: rf = variance, cf = 1). The sum(u^2) pass takes its norm and the apply pass
// applies it: both call this one function, compiled without contraction, so the clipped norm is
// exactly the norm of what is applied.
__device__ __forceinline__ float af_dir(float gg, float rf, float cf, float e2) {
#pragma clang fp contract(off)
  const float v = af_floor(rf * cf, e2);
  return rsqrtf(v) * gg;
}

__device__ __forceinline__ float af_gscale(const AfArgs& a) {
  return (a.gs ? *a.gs : 1.f) * (a.maximize ? -1.f : 1.f);
}

// ---- 1. tile statistics --------------------------------------------------------------
template <typename W, typename G>
__global__ __launch_bounds__(kThreads) void af_stats_kernel(MatTable t, AfArgs a) {
  __shared__ float cpart[kRowGroups][kTC];
  __shared__ float red[kThreads / 64];
  const Tile q = block_tile(t);
  const Mat m(reinterpret_cast<float*>(t.ptr[4][q.s]), t.B[q.s], t.R[q.s], t.C[q.s]);
  const int64_t plane = (int64_t)q.b * m.R * m.C;
  const W* w = reinterpret_cast<const W*>(t.ptr[0][q.s]) + plane;
  const G* g = reinterpret_cast<const G*>(t.ptr[1][q.s]) + plane;
  const bool vec = (t.vec >> q.s) & 1;
  const int lane = threadIdx.x % kLanesC, rg = threadIdx.x / kLanesC;
  const int col0 = q.ct * kTC + lane * 8;
  const float gscale = af_gscale(a);
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float sw = 0.f;
#pragma unroll 2
  for (int k = 0; k < kRowIters; ++k) {
    const int row = q.rt * kTR + k * kRowGroups + rg;
    float gv[8], wv[8];
    ld_row8(g, row, col0, m.R, m.C, vec, gv);
    ld_row8(w, row, col0, m.R, m.C, vec, wv);
    float rs = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float gg = gv[j] * gscale;
      const float sq = gg * gg;
      cs[j] += sq;
      rs += sq;
      sw = fmaf(wv[j], wv[j], sw);
    }
#pragma unroll
    for (int o = kLanesC / 2; o > 0; o >>= 1) rs += __shfl_xor(rs, o, 64);  // stays in the row's 32 lanes
    if (lane == 0 && row < m.R) m.rowp()[((int64_t)q.b * m.R + row) * m.nCT + q.ct] = rs;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) cpart[rg][lane * 8 + j] = cs[j];
  __syncthreads();
  float c = 0.f;
#pragma unroll
  for (int r = 0; r < kRowGroups; ++r) c += cpart[r][threadIdx.x];
  const int col = q.ct * kTC + threadIdx.x;
  if (col < m.C) m.colp()[((int64_t)q.b * m.nRT + q.rt) * m.C + col] = c;
  sw = dev::block_sum(sw, red);
  if (threadIdx.x == 0) m.wsq()[q.tl] = sw;
}

// ---- 2. fold the partials into the factors -------------------------------------------
__global__ __launch_bounds__(kThreads) void af_fold_kernel(MatTable t, AfArgs a) {
  __shared__ double red[kThreads / 64];
  const int s = find_end(t.fold_end, t.nseg, blockIdx.x);
  const int f = blockIdx.x - (s ? t.fold_end[s - 1] : 0);
  const Mat m(reinterpret_cast<float*>(t.ptr[4][s]), t.B[s], t.R[s], t.C[s]);
  const int b = f / (m.nRB + m.nCB), q = f % (m.nRB + m.nCB);
  if (q >= m.nRB) {  // 256 columns of matrix b
    const int col = (q - m.nRB) * kFoldCols + threadIdx.x;
    if (col >= m.C) return;
    const float* p = m.colp() + (int64_t)b * m.nRT * m.C + col;
    double sum = 0.0;
    for (int rt = 0; rt < m.nRT; ++rt) sum += (double)p[(int64_t)rt * m.C];
    float* cv = reinterpret_cast<float*>(t.ptr[3][s]) + (int64_t)b * m.C + col;
    *cv = af_lerp(*cv, (float)(sum / (double)m.R), a.omb);
    return;
  }
  // 2048 rows of matrix b, and the sum of their new row_var
  float* rv = reinterpret_cast<float*>(t.ptr[2][s]) + (int64_t)b * m.R;
  const int end = min(m.R, (q + 1) * kFoldRows);
  double acc = 0.0;
  for (int row = q * kFoldRows + threadIdx.x; row < end; row += kThreads) {
    const float* p = m.rowp() + ((int64_t)b * m.R + row) * m.nCT;
    double sum = 0.0;
    for (int ct = 0; ct < m.nCT; ++ct) sum += (double)p[ct];
    const float v = af_lerp(rv[row], (float)(sum / (double)m.C), a.omb);
    rv[row] = v;
    acc += (double)v;
  }
  acc = dev::block_sum(acc, red);
  if (threadIdx.x == 0) m.rvp()[(int64_t)b * m.nRB + q] = (float)acc;
}

// ---- 3. sum(u^2) per tile, 5. the update ---------------------------------------------
// What both passes share: the tile's factors, and u of one row
struct TileDir {
  float cf[8];
  float rm, e2, gscale;
  __device__ __forceinline__ TileDir(const MatTable& t, const Tile& q, const Mat& m, int col0, const AfArgs& a)
      : e2(a.e2), gscale(af_gscale(a)) {
    // max(mean row_var, eps1): the matrix's fold-block sums in block order, the same in every tile
    const float* part = m.rvp() + (int64_t)q.b * m.nRB;
    double sum = 0.0;
    for (int i = 0; i < m.nRB; ++i) sum += (double)part[i];
    rm = af_floor((float)(sum / (double)m.R), a.eps1);
    const float* cv = reinterpret_cast<const float*>(t.ptr[3][q.s]) + (int64_t)q.b * m.C;
#pragma unroll
    for (int j = 0; j < 8; ++j) cf[j] = col0 + j < m.C ? cv[col0 + j] : 0.f;
  }
  // row_var / max(mean row_var, eps1) of one row
  __device__ __forceinline__ float row_factor(const float* rv, int row, int R) const {
    return row < R ? rv[row] / rm : 0.f;
  }
  __device__ __forceinline__ void dir(const float (&gv)[8], float rf, float (&u)[8]) const {
#pragma unroll
    for (int j = 0; j < 8; ++j) u[j] = af_dir(gv[j] * gscale, rf, cf[j], e2);
  }
};

template <typename G>
__global__ __launch_bounds__(kThreads) void af_usq_kernel(MatTable t, AfArgs a) {
  __shared__ float red[kThreads / 64];
  const Tile q = block_tile(t);
  const Mat m(reinterpret_cast<float*>(t.ptr[4][q.s]), t.B[q.s], t.R[q.s], t.C[q.s]);
  const G* g = reinterpret_cast<const G*>(t.ptr[1][q.s]) + (int64_t)q.b * m.R * m.C;
  const float* rv = reinterpret_cast<const float*>(t.ptr[2][q.s]) + (int64_t)q.b * m.R;
  const bool vec = (t.vec >> q.s) & 1;
  const int lane = threadIdx.x % kLanesC, rg = threadIdx.x / kLanesC;
  const int col0 = q.ct * kTC + lane * 8;
  const TileDir td(t, q, m, col0, a);
  float su = 0.f;
#pragma unroll 2
  for (int k = 0; k < kRowIters; ++k) {
    const int row = q.rt * kTR + k * kRowGroups + rg;
    float gv[8], u[8];
    ld_row8(g, row, col0, m.R, m.C, vec, gv);
    td.dir(gv, td.row_factor(rv, row, m.R), u);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (row < m.R && col0 + j < m.C) su = fmaf(u[j], u[j], su);  // (outside, u may be 0 * inf)
  }
  su = dev::block_sum(su, red);
  if (threadIdx.x == 0) m.usq()[q.tl] = su;
}

// ---- 4. alpha / max(1, RMS(u) / d), one block per tensor -----------------------------
__global__ __launch_bounds__(kThreads) void af_coef_kernel(MatTable t, AfArgs a) {
  __shared__ double red[kThreads / 64];
  const int s = blockIdx.x;
  const Mat m(reinterpret_cast<float*>(t.ptr[4][s]), t.B[s], t.R[s], t.C[s]);
  double su = 0.0;
  for (int64_t i = threadIdx.x; i < m.tiles; i += kThreads) su += (double)m.usq()[i];
  su = dev::block_sum(su, red);
  double sw = 0.0;  // alpha = max(eps2, RMS(w)) rho, of w before the decay
  for (int64_t i = threadIdx.x; i < m.tiles; i += kThreads) sw += (double)m.wsq()[i];
  sw = dev::block_sum(sw, red);
  if (threadIdx.x != 0) return;
  const double n = (double)m.B * m.R * m.C;
  const double alpha = fmax((double)a.eps2, sqrt(sw / n)) * (double)a.rho;
  const double r = sqrt(su / n) / (double)a.d;
  *m.coef() = (float)(alpha / (r < 1.0 ? 1.0 : r));  // (a NaN norm stays NaN)
}

template <typename P, typename G, bool MASTER>
__global__ __launch_bounds__(kThreads) void af_apply_kernel(MatTable t, AfArgs a) {
  using W = std::conditional_t<MASTER, float, P>;
  const Tile q = block_tile(t);
  const Mat m(reinterpret_cast<float*>(t.ptr[4][q.s]), t.B[q.s], t.R[q.s], t.C[q.s]);
  const int64_t plane = (int64_t)q.b * m.R * m.C;
  W* w = reinterpret_cast<W*>(t.ptr[0][q.s]) + plane;
  const G* g = reinterpret_cast<const G*>(t.ptr[1][q.s]) + plane;
  const float* rv = reinterpret_cast<const float*>(t.ptr[2][q.s]) + (int64_t)q.b * m.R;
  P* p = nullptr;
  if constexpr (MASTER) p = reinterpret_cast<P*>(t.ptr[5][q.s]) + plane;
  const bool vec = (t.vec >> q.s) & 1;
  const int lane = threadIdx.x % kLanesC, rg = threadIdx.x / kLanesC;
  const int col0 = q.ct * kTC + lane * 8;
  const TileDir td(t, q, m, col0, a);
  const float step = -*m.coef();
#pragma unroll 2
  for (int k = 0; k < kRowIters; ++k) {
    const int row = q.rt * kTR + k * kRowGroups + rg;
    float gv[8], wv[8], u[8];
    ld_row8(g, row, col0, m.R, m.C, vec, gv);
    ld_row8(w, row, col0, m.R, m.C, vec, wv);
    td.dir(gv, td.row_factor(rv, row, m.R), u);
#pragma unroll
    for (int j = 0; j < 8; ++j) wv[j] = fmaf(step, u[j], wv[j] * a.decay);
    st_row8(w, row, col0, m.R, m.C, vec, wv);
    if constexpr (MASTER) st_row8(p, row, col0, m.R, m.C, vec, wv);
  }
}

// ---- parameters of dim <= 1: the flat three-stage pattern ----------------------------
// Stage 1, slots {w, grad, variance, this tensor's chunk partials}: variance <- lerp(variance, g'^2),
// and sum(w^2), sum(u^2) of the chunk.
template <typename W, typename G, bool VEC>
__global__ __launch_bounds__(kThreads) void af_vec_stats_kernel(SegTable<4> t, AfArgs a) {
  __shared__ float red[kThreads / 64];
  const Chunk c = block_chunk(t);
  const W* w = reinterpret_cast<const W*>(t.ptr[0][c.s]);
  const G* g = reinterpret_cast<const G*>(t.ptr[1][c.s]);
  float* var = reinterpret_cast<float*>(t.ptr[2][c.s]);
  float* part = reinterpret_cast<float*>(t.ptr[3][c.s]) + 2 * (c.base / kChunk);
  const float gscale = af_gscale(a);
  float sw = 0.f, su = 0.f;
  auto upd = [&](float wv, float gv, float& vv) {
    const float gg = gv * gscale;
    vv = af_lerp(vv, gg * gg, a.omb);
    const float u = af_dir(gg, vv, 1.f, a.e2);
    sw = fmaf(wv, wv, sw);
    su = fmaf(u, u, su);
  };
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int64_t i = c.base + ((int64_t)it * kThreads + threadIdx.x) * 8;
    if (VEC && i + 8 <= c.n) {
      float wv[8], gv[8], vv[8];
      Vec8<W>::ld(w + i, wv);
      Vec8<G>::ld(g + i, gv);
      Vec8<float>::ld(var + i, vv);
#pragma unroll
      for (int j = 0; j < 8; ++j) upd(wv[j], gv[j], vv[j]);
      Vec8<float>::st(var + i, vv);
    } else {
      for (int64_t k = i; k < i + 8 && k < c.n; ++k) {
        float vv = var[k];
        upd(Elem<W, float>::ld(w, k), Elem<G, float>::ld(g, k), vv);
        var[k] = vv;
      }
    }
  }
  sw = dev::block_sum(sw, red);
  su = dev::block_sum(su, red);
  if (threadIdx.x == 0) {
    part[0] = sw;
    part[1] = su;
  }
}

// Stage 2, slots {this tensor's chunk partials, the address of its coefficient}; "numel" is the
// tensor's. Block s is tensor s; one wave folds the chunk partials in a fixed order.
__global__ __launch_bounds__(64) void af_vec_coef_kernel(SegTable<2> t, AfArgs a) {
  const int s = blockIdx.x;
  const float* part = reinterpret_cast<const float*>(t.ptr[0][s]);
  const int64_t n = t.numel[s], chunks = (n + kChunk - 1) / kChunk;
  double sw = 0.0, su = 0.0;
  for (int64_t i = threadIdx.x; i < chunks; i += 64) {
    sw += (double)part[2 * i];
    su += (double)part[2 * i + 1];
  }
  sw = dev::wave_sum(sw);
  su = dev::wave_sum(su);
  if (threadIdx.x != 0) return;
  const double alpha = fmax((double)a.eps2, sqrt(sw / (double)n)) * (double)a.rho;
  const double r = sqrt(su / (double)n) / (double)a.d;
  *reinterpret_cast<float*>(t.ptr[1][s]) = (float)(alpha / (r < 1.0 ? 1.0 : r));
}

// Stage 3, slots {w, grad, variance, the address of the tensor's coefficient, the model's parameter (MASTER)}
template <typename P, typename G, bool VEC, bool MASTER>
__global__ __launch_bounds__(kThreads) void af_vec_apply_kernel(SegTable<5> t, AfArgs a) {
  using W = std::conditional_t<MASTER, float, P>;
  const Chunk c = block_chunk(t);
  W* w = reinterpret_cast<W*>(t.ptr[0][c.s]);
  const G* g = reinterpret_cast<const G*>(t.ptr[1][c.s]);
  const float* var = reinterpret_cast<const float*>(t.ptr[2][c.s]);
  const float step = -*reinterpret_cast<const float*>(t.ptr[3][c.s]);
  P* p = nullptr;
  if constexpr (MASTER) p = reinterpret_cast<P*>(t.ptr[4][c.s]);
  const float gscale = af_gscale(a);
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int64_t i = c.base + ((int64_t)it * kThreads + threadIdx.x) * 8;
    if (VEC && i + 8 <= c.n) {
      float wv[8], gv[8], vv[8];
      Vec8<W>::ld(w + i, wv);
      Vec8<G>::ld(g + i, gv);
      Vec8<float>::ld(var + i, vv);
#pragma unroll
      for (int j = 0; j < 8; ++j) wv[j] = fmaf(step, af_dir(gv[j] * gscale, vv[j], 1.f, a.e2), wv[j] * a.decay);
      Vec8<W>::st(w + i, wv);
      if (MASTER) Vec8<P>::st(p + i, wv);
    } else {
      for (int64_t k = i; k < i + 8 && k < c.n; ++k) {
        const float gg = Elem<G, float>::ld(g, k) * gscale;
        const float wv = fmaf(step, af_dir(gg, var[k], 1.f, a.e2), Elem<W, float>::ld(w, k) * a.decay);
        Elem<W, float>::st(w, k, wv);
        if (MASTER) Elem<P, float>::st(p, k, wv);
      }
    }
  }
}

// ---- host ----------------------------------------------------------------------------
static void check_f32(const char* what, const at::Tensor& x, int64_t numel) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.is_contiguous() && x.numel() == numel,
              "fused_adafactor: ", what, " must be a contiguous fp32 device tensor of ", numel, " elements");
}

template <typename K>
static void launch_mat(K kernel, int blocks, const MatTable& t, const AfArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kThreads), 0, stream, t, a);
  XDDP_HIP_CHECK(hipGetLastError());
}

// The five launches of one table
static void step_table(const MatTable& t, const AfArgs& a, at::ScalarType pt, at::ScalarType gt, bool has_master,
                       hipStream_t stream) {
  const int tiles = t.tile_end[t.nseg - 1], folds = t.fold_end[t.nseg - 1];
  const auto wt = has_master ? at::kFloat : pt;
  XDDP_DISPATCH_FLOAT_NO_F64(gt, G, "fused Adafactor: unsupported gradient dtype ", {
    XDDP_DISPATCH_FLOAT_NO_F64(wt, W, "fused Adafactor: unsupported parameter dtype ",
                               { launch_mat(af_stats_kernel<W, G>, tiles, t, a, stream); });
    launch_mat(af_fold_kernel, folds, t, a, stream);
    launch_mat(af_usq_kernel<G>, tiles, t, a, stream);
    launch_mat(af_coef_kernel, t.nseg, t, a, stream);
    XDDP_DISPATCH_FLOAT_NO_F64(pt, P, "fused Adafactor: unsupported parameter dtype ", {
      if (has_master) {
        if constexpr (!std::is_same<P, float>::value) launch_mat(af_apply_kernel<P, G, true>, tiles, t, a, stream);
      } else {
        launch_mat(af_apply_kernel<P, G, false>, tiles, t, a, stream);
      }
    });
  });
}

static void adafactor_matrices(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                               const std::vector<at::Tensor>& row_vars, const std::vector<at::Tensor>& col_vars,
                               const std::vector<at::Tensor>& masters, const AfArgs& a, hipStream_t stream) {
  const size_t N = params.size();
  const bool has_master = !masters.empty();
  const auto pt = params[0].scalar_type(), gt = grads[0].scalar_type();
  struct Dims {
    int B, R, C;
    int64_t off;
  };
  std::vector<Dims> dims(N);
  int64_t total = 0;
  for (size_t i = 0; i < N; ++i) {
    const at::Tensor& p = params[i];
    TORCH_CHECK(p.dim() >= 2, "fused_adafactor: a list of matrices holds tensors of dim >= 2 only");
    const int64_t R = p.size(-2), C = p.size(-1);
    int64_t B = 1;
    for (int64_t k = 0; k + 2 < p.dim(); ++k) B *= p.size(k);
    TORCH_CHECK(R < (1ll << 31) && C < (1ll << 31) && B < (1ll << 31), "fused_adafactor: dimension too large");
    check_f32("row_var", row_vars[i], B * R);
    check_f32("col_var", col_vars[i], B * C);
    dims[i] = {(int)B, (int)R, (int)C, total};
    if (p.numel() == 0) continue;
    const Mat m(nullptr, (int)B, (int)R, (int)C);
    TORCH_CHECK(m.tiles < (1ll << 30) && m.fold_blocks() < (1ll << 30), "fused_adafactor: tensor too large");
    total += (m.scratch_floats() + 3) / 4 * 4;
  }
  at::Tensor scratch = at::empty({std::max<int64_t>(total, 1)},
                                 at::TensorOptions().dtype(at::kFloat).device(params[0].device()));
  float* sbase = scratch.data_ptr<float>();
  MatTable t;
  t.nseg = 0;
  t.vec = 0;
  int64_t tiles = 0, folds = 0;
  for (size_t i = 0; i < N; ++i) {
    if (params[i].numel() == 0) continue;
    const Mat m(sbase + dims[i].off, dims[i].B, dims[i].R, dims[i].C);
    if (t.nseg == kMaxSeg || tiles + m.tiles > (1ll << 30) || folds + m.fold_blocks() > (1ll << 30)) {
      step_table(t, a, pt, gt, has_master, stream);
      t.nseg = 0;
      t.vec = 0;
      tiles = folds = 0;
    }
    const int s = t.nseg++;
    void* w = has_master ? masters[i].data_ptr() : params[i].data_ptr();
    void* g = const_cast<void*>(grads[i].data_ptr());
    void* p = has_master ? params[i].data_ptr() : nullptr;
    t.ptr[0][s] = w;
    t.ptr[1][s] = g;
    t.ptr[2][s] = row_vars[i].data_ptr();
    t.ptr[3][s] = col_vars[i].data_ptr();
    t.ptr[4][s] = sbase + dims[i].off;
    t.ptr[5][s] = p;
    t.B[s] = m.B, t.R[s] = m.R, t.C[s] = m.C;
    if (m.C % 8 == 0 && aligned16(w) && aligned16(g) && aligned16(p)) t.vec |= 1ull << s;
    tiles += m.tiles;
    folds += m.fold_blocks();
    t.tile_end[s] = (int32_t)tiles;
    t.fold_end[s] = (int32_t)folds;
  }
  if (t.nseg) step_table(t, a, pt, gt, has_master, stream);
}

static void adafactor_vectors(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                              const std::vector<at::Tensor>& variances, const std::vector<at::Tensor>& masters,
                              const AfArgs& a, hipStream_t stream) {
  const size_t N = params.size();
  const bool has_master = !masters.empty();
  const auto pt = params[0].scalar_type(), gt = grads[0].scalar_type();
  std::vector<int64_t> start(N), numels(N);
  int64_t chunks = 0;
  for (size_t i = 0; i < N; ++i) {
    TORCH_CHECK(params[i].dim() <= 1, "fused_adafactor: a list of vectors holds tensors of dim <= 1 only");
    check_f32("variance", variances[i], params[i].numel());
    numels[i] = params[i].numel();
    start[i] = chunks;
    chunks += (numels[i] + kChunk - 1) / kChunk;
  }
  const auto f32 = at::TensorOptions().dtype(at::kFloat).device(params[0].device());
  at::Tensor partials = at::empty({2 * std::max<int64_t>(chunks, 1)}, f32);
  at::Tensor coefs = at::empty({(int64_t)N}, f32);
  float* part = partials.data_ptr<float>();
  float* coef = coefs.data_ptr<float>();
  std::vector<std::array<void*, 4>> p1;
  std::vector<std::array<void*, 5>> p3;
  bool vec1 = true, vec3 = true;
  for (size_t i = 0; i < N; ++i) {
    void* w = has_master ? masters[i].data_ptr() : params[i].data_ptr();
    void* g = const_cast<void*>(grads[i].data_ptr());
    void* v = variances[i].data_ptr();
    void* p = has_master ? params[i].data_ptr() : nullptr;
    p1.push_back({w, g, v, part + 2 * start[i]});
    p3.push_back({w, g, v, coef + i, p});
    vec1 = vec1 && aligned16(w) && aligned16(g) && aligned16(v);
    vec3 = vec3 && aligned16(w) && aligned16(g) && aligned16(v) && aligned16(p);
  }
  const auto wt = has_master ? at::kFloat : pt;
  XDDP_DISPATCH_FLOAT_NO_F64(gt, G, "fused Adafactor: unsupported gradient dtype ", {
    XDDP_DISPATCH_FLOAT_NO_F64(wt, W, "fused Adafactor: unsupported parameter dtype ", {
      launch_list<4>(vec1 ? af_vec_stats_kernel<W, G, true> : af_vec_stats_kernel<W, G, false>, p1, numels, a, stream);
    });
    SegTable<2> t;  // stage 2: tensor s of the table is block s
    t.nseg = 0;
    auto flush = [&]() {
      hipLaunchKernelGGL(af_vec_coef_kernel, dim3(t.nseg), dim3(64), 0, stream, t, a);
      XDDP_HIP_CHECK(hipGetLastError());
      t.nseg = 0;
    };
    for (size_t i = 0; i < N; ++i) {
      if (numels[i] == 0) continue;
      t.ptr[0][t.nseg] = part + 2 * start[i];
      t.ptr[1][t.nseg] = coef + i;
      t.numel[t.nseg] = numels[i];
      t.blk_end[t.nseg] = t.nseg + 1;
      if (++t.nseg == kMaxSeg) flush();
    }
    if (t.nseg) flush();
    XDDP_DISPATCH_FLOAT_NO_F64(pt, P, "fused Adafactor: unsupported parameter dtype ", {
      if (has_master) {
        if constexpr (!std::is_same<P, float>::value)
          launch_list<5>(vec3 ? af_vec_apply_kernel<P, G, true, true> : af_vec_apply_kernel<P, G, false, true>, p3,
                         numels, a, stream);
      } else {
        launch_list<5>(vec3 ? af_vec_apply_kernel<P, G, true, false> : af_vec_apply_kernel<P, G, false, false>, p3,
                       numels, a, stream);
      }
    });
  });
}

void fused_adafactor(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                     const std::vector<at::Tensor>& row_vars, const std::vector<at::Tensor>& col_vars,
                     const std::vector<at::Tensor>& variances, const std::vector<at::Tensor>& masters, double lr,
                     double beta2_decay, double eps1, double eps2, double d, double weight_decay, int64_t step,
                     bool maximize, const c10::optional<at::Tensor>& grad_scale, hipStream_t stream) {
  const size_t N = params.size();
  TORCH_CHECK(N > 0, "fused_adafactor: empty tensor list");
  const bool matrices = !row_vars.empty() || !col_vars.empty();
  TORCH_CHECK(grads.size() == N && (matrices ? row_vars.size() == N && col_vars.size() == N && variances.empty()
                                             : variances.size() == N),
              "fused_adafactor: list length mismatch (row_vars and col_vars for matrices, or variances for vectors)");
  const bool has_master = !masters.empty();
  TORCH_CHECK(!has_master || masters.size() == N, "fused_adafactor: masters length mismatch");
  TORCH_CHECK(step >= 1, "fused_adafactor: step must be >= 1");
  TORCH_CHECK(d >= 1.0 && eps1 >= 0.0 && eps2 >= 0.0, "fused_adafactor: d >= 1, eps1 >= 0 and eps2 >= 0 expected");
  const auto pt = params[0].scalar_type(), gt = grads[0].scalar_type();
  TORCH_CHECK(pt != at::kDouble && gt != at::kDouble, "fused Adafactor: fp64 unsupported");
  TORCH_CHECK(!has_master || pt == at::kBFloat16 || pt == at::kHalf,
              "master-weight Adafactor: model params must be bf16/fp16");
  for (size_t i = 0; i < N; ++i) {
    const at::Tensor &p = params[i], &g = grads[i];
    TORCH_CHECK(p.is_cuda() && g.is_cuda() && p.scalar_type() == pt && g.scalar_type() == gt,
                "fused_adafactor: device tensors of one dtype per list expected");
    TORCH_CHECK(p.is_contiguous() && g.is_contiguous() && p.sizes() == g.sizes(),
                "fused_adafactor: parameters and gradients must be contiguous (row-major) and of one shape");
    if (has_master)
      TORCH_CHECK(masters[i].is_cuda() && masters[i].scalar_type() == at::kFloat && masters[i].is_contiguous() &&
                      masters[i].sizes() == p.sizes(),
                  "fused_adafactor: master weights must be contiguous fp32 of the parameter's shape");
  }
  const double t = (double)step;
  const AfArgs a = {(float)std::pow(t, beta2_decay), (float)std::min(lr, 1.0 / std::sqrt(t)), (float)eps1,
                    (float)(eps1 * eps1), (float)eps2, (float)d, (float)(1.0 - lr * weight_decay), maximize,
                    scale_ptr(grad_scale)};
  if (matrices) adafactor_matrices(params, grads, row_vars, col_vars, masters, a, stream);
  else adafactor_vectors(params, grads, variances, masters, a, stream);
}

}  // namespace kernels
}  // namespace xddp
