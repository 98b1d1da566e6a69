// Fused PowerSGD (Vogels et al. 2019; the arithmetic of comm_hooks/powerSGD_hook.py) for gfx950.
//
// A bucket's compressible gradients are row-major [n, m] views G of the flat bucket (fp32, bf16 or
// fp16; any base alignment, any m), each with an fp32 error memory E, P [n, r] and Q [m, r],
// r = min(n, m, rank) <= 32. The three products are tall-skinny (r / 2 flop per byte): streaming
// kernels with the small operand in LDS, no MFMA. Up to kMaxSeg matrices share a launch through a
// by-value table; the kernels are instantiated on the padded rank RP (1, 2, 4, 8, 16, 32) and guard
// on k < r, and a list is grouped by RP. M' = G + E is formed in registers and never written.
//
//   psgd_project_kernel      P = M' Q. A block owns a 32 x 256 tile; the Q rows of its 256 columns
//                            sit in LDS, transposed. A row is spread over 32 lanes of 8 columns each
//                            and a thread works on two rows at once (one LDS read of Q feeds both).
//                            The RP sums of a row fold across its 32 lanes with a halving butterfly:
//                            at each __shfl_xor step a lane gives away half of its values, so the
//                            fold costs RP - 1 shuffles (not 5 RP) and leaves sum k on lane
//                            k * 32 / RP, which writes it. With more than one column tile the
//                            block writes slot [column tile][n][r] and psgd_fold_kernel sums the
//                            slots in tile order: a 10 x 4096 matrix runs on 16 blocks (64 waves).
//   psgd_gram_kernel         X^T X of 256 rows of X [n, r] from LDS into slot [row block][RP][RP];
//   psgd_chol_kernel         one wave per matrix: folds the slots in order, regularises, r x r
//                            Cholesky and the inverse of L by forward substitution in LDS, fp32;
//   psgd_apply_kernel        X <- X L^-T, a thread per row, L^-T broadcast from LDS.
//                            CholeskyQR2 is these three twice: six launches per table.
//   psgd_backproject_kernel  Q = M'^T P. A thread owns CW = min(8, 64 / RP) consecutive columns and
//                            CW * RP <= 64 accumulators over the rows of its row group (8 groups of
//                            32 lanes); the tile's P rows are broadcast from LDS. The 8 groups fold
//                            through LDS as a fixed tree; with more than one row tile (64 rows, 128 at
//                            RP = 32) the block writes slot [row tile][m][r], folded in tile order.
//   psgd_reconstruct_kernel  A = inv_world P Q^T rounded to the bucket dtype, E <- (G + E) - A,
//                            G <- A: a 32 x 256 tile, 4 rows x 8 columns per thread, k outermost so
//                            that one LDS read of 8 Q values feeds 32 FMAs.
//
// Every partial has its own slot and every fold a fixed order; no float atomics, no host
// synchronisation. Tile geometry depends on (n, m, r) alone, so a matrix's result is bitwise the same
// alone, in any list and on every replica (the file is built without packed fp32 operations).
#include "kernels/powersgd.h"

#include <ATen/hip/HIPContext.h>

#include <algorithm>

#include "common.h"
#include "kernels/dev_utils.h"
#include "kernels/mt_common.h"

namespace xddp {
namespace kernels {

namespace {

constexpr int kLanes = 32;                  // lanes across a tile row
constexpr int kRG = kThreads / kLanes;      // row groups of a block
constexpr int kPR = 32, kPC = kLanes * 8;   // the tile of project and reconstruct
constexpr int kOR = kThreads;               // rows per block of the Gram and apply kernels
constexpr int kMaxRank = 32;
static_assert(kRG == 8 && kPR % (2 * kRG) == 0, "two rows per thread and pass");

// columns a thread of the backproject kernel owns, and the rows of its tile
template <int RP> constexpr int kBackCW = RP <= 8 ? 8 : 64 / RP;
template <int RP> constexpr int kBackRows = RP == 32 ? 128 : 64;

// What the slots mean is the kernel's business (see each kernel); `n`, `m`, `r` are the matrix's.
struct PsgdTable {
  void* g[kMaxSeg];
  float* e[kMaxSeg];
  float* p[kMaxSeg];
  float* q[kMaxSeg];
  float* ws[kMaxSeg];
  int32_t n[kMaxSeg], m[kMaxSeg], r[kMaxSeg];
  int32_t blk_end[kMaxSeg];  // inclusive prefix sums of blocks per segment
  uint64_t vec;              // bit s: G and E of segment s are 16-byte aligned and m % 8 == 0
  int32_t nseg;
};
static_assert(kMaxSeg <= 64, "one bit per segment");
static_assert(sizeof(PsgdTable) + 64 <= 4096, "the by-value table must fit the kernarg segment");

struct Seg {
  int s, blk;
};
__device__ __forceinline__ Seg block_seg(const PsgdTable& t) {
  int lo = 0, hi = t.nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int)blockIdx.x < t.blk_end[mid]) hi = mid; else lo = mid + 1;
  }
  return {lo, (int)blockIdx.x - (lo ? t.blk_end[lo - 1] : 0)};
}

// W consecutive elements from `off`, of which `valid` (<= 0: none) are inside the row; 0 outside
template <typename T, int W>
__device__ __forceinline__ void ld_cols(const T* base, int64_t off, int valid, bool vec, float (&v)[W]) {
  if (vec && valid >= W) {
    constexpr int kAlign = W * sizeof(T) > 16 ? 16 : W * sizeof(T);
    T tmp[W];
    __builtin_memcpy(tmp, __builtin_assume_aligned(base + off, kAlign), sizeof(tmp));
#pragma unroll
    for (int j = 0; j < W; ++j) v[j] = Elem<T, float>::ld(tmp, j);
  } else {
#pragma unroll
    for (int j = 0; j < W; ++j) v[j] = j < valid ? Elem<T, float>::ld(base, off + j) : 0.f;
  }
}
template <typename T, int W>
__device__ __forceinline__ void st_cols(T* base, int64_t off, int valid, bool vec, const float (&v)[W]) {
  if (vec && valid >= W) {
    constexpr int kAlign = W * sizeof(T) > 16 ? 16 : W * sizeof(T);
    T tmp[W];
#pragma unroll
    for (int j = 0; j < W; ++j) Elem<T, float>::st(tmp, j, v[j]);
    __builtin_memcpy(__builtin_assume_aligned(base + off, kAlign), tmp, sizeof(tmp));
  } else {
#pragma unroll
    for (int j = 0; j < W; ++j)
      if (j < valid) Elem<T, float>::st(base, off + j, v[j]);
  }
}
// M' = G + E of W elements (E = 0 without error feedback)
template <typename T, int W>
__device__ __forceinline__ void ld_m(const T* g, const float* e, int64_t off, int valid, bool vec, float (&v)[W]) {
  ld_cols<T, W>(g, off, valid, vec, v);
  if (e) {
    float ev[W];
    ld_cols<float, W>(e, off, valid, vec, ev);
#pragma unroll
    for (int j = 0; j < W; ++j) v[j] += ev[j];
  }
}

// Sums v[k] over the 32 lanes of a row. Step s (lane distance 16 >> s) halves the values a lane
// holds while there is more than one: the upper lane of a pair keeps the upper half. Returns the
// k whose total ends in v[0]; lanes that differ only in the low log2(32 / RP) bits hold the same.
template <int RP, int S>
__device__ __forceinline__ void fold_step(float (&v)[RP], int lane, int& kidx) {
  constexpr int o = (kLanes / 2) >> S, cnt = RP >> S;
  if constexpr (cnt > 1) {
    constexpr int half = cnt / 2;
    const bool up = (lane & o) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const float send = up ? v[i] : v[i + half];
      const float keep = up ? v[i + half] : v[i];
      v[i] = keep + __shfl_xor(send, o, 64);
    }
    kidx += up ? half : 0;
  } else {
    v[0] += __shfl_xor(v[0], o, 64);
  }
  if constexpr (S < 4) fold_step<RP, S + 1>(v, lane, kidx);
}
template <int RP>
__device__ __forceinline__ int fold_row(float (&v)[RP], int lane) {
  int kidx = 0;
  fold_step<RP, 0>(v, lane, kidx);
  return kidx;
}

// The Q rows of the tile's columns, transposed: qs[k][c] = Q[ct * kPC + c][k], 0 outside
template <int RP>
__device__ __forceinline__ void fill_qs(float (&qs)[RP][kPC + 4], const float* q, int ct, int m, int r) {
  for (int idx = threadIdx.x; idx < kPC * RP; idx += kThreads) {
    const int c = idx / RP, k = idx % RP, col = ct * kPC + c;
    qs[k][c] = (k < r && col < m) ? q[(int64_t)col * r + k] : 0.f;
  }
}
// Rows [row0, row0 + ROWS) of X [n, r]: xs[i][k], 0 outside
template <int ROWS, int RP>
__device__ __forceinline__ void fill_rows(float (&xs)[ROWS][RP], const float* x, int64_t row0, int n, int r) {
  for (int idx = threadIdx.x; idx < ROWS * RP; idx += blockDim.x) {
    const int i = idx / RP, k = idx % RP;
    xs[i][k] = (k < r && row0 + i < n) ? x[(row0 + i) * r + k] : 0.f;
  }
}

// ---- P = M' Q ------------------------------------------------------------------------
// Slots: g, e, q; p = where the tile's sums go: P itself (one column tile) or the partial slab
// [column tiles][n][r].
template <typename T, int RP>
__global__ __launch_bounds__(kThreads) void psgd_project_kernel(PsgdTable t) {
  __shared__ __attribute__((aligned(16))) float qs[RP][kPC + 4];
  const Seg b = block_seg(t);
  const int n = t.n[b.s], m = t.m[b.s], r = t.r[b.s];
  const int nCT = (m + kPC - 1) / kPC, rt = b.blk / nCT, ct = b.blk % nCT;
  const T* g = reinterpret_cast<const T*>(t.g[b.s]);
  const float* e = t.e[b.s];
  float* dst = t.p[b.s] + (int64_t)ct * n * r;  // (ct = 0 with one column tile)
  const bool vec = (t.vec >> b.s) & 1;
  fill_qs<RP>(qs, t.q[b.s], ct, m, r);
  __syncthreads();
  const int lane = threadIdx.x % kLanes, rg = threadIdx.x / kLanes;
  const int col0 = ct * kPC + lane * 8;
#pragma unroll 1
  for (int pass = 0; pass < kPR / (2 * kRG); ++pass) {
    const int row[2] = {rt * kPR + pass * 2 * kRG + rg, rt * kPR + pass * 2 * kRG + kRG + rg};
    float mv[2][8], acc[2][RP];
#pragma unroll
    for (int i = 0; i < 2; ++i)
      ld_m<T, 8>(g, e, (int64_t)row[i] * m + col0, row[i] < n ? m - col0 : 0, vec, mv[i]);
#pragma unroll
    for (int k = 0; k < RP; ++k) {
      const dev::f32x4 qa = *reinterpret_cast<const dev::f32x4*>(&qs[k][lane * 8]);
      const dev::f32x4 qb = *reinterpret_cast<const dev::f32x4*>(&qs[k][lane * 8 + 4]);
      const float q8[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a = fmaf(mv[i][j], q8[j], a);
        acc[i][k] = a;
      }
      // both rows' sums exist here: sunk below the first row's fold, the second row's FMAs would
      // keep all 8 RP values of Q in registers
      asm volatile("" : "+v"(acc[0][k]), "+v"(acc[1][k]));
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int k = fold_row<RP>(acc[i], lane);  // (every lane of the wave takes part)
      if (lane % (kLanes / RP) == 0 && k < r && row[i] < n) dst[(int64_t)row[i] * r + k] = acc[i][0];
    }
  }
}

// out[i] = sum over the slots, in slot order. Slots: p = out, ws = slots; n = the length of out and
// of a slot, m = the number of slots.
__global__ __launch_bounds__(kThreads) void psgd_fold_kernel(PsgdTable t) {
  const Seg b = block_seg(t);
  const int len = t.n[b.s], slots = t.m[b.s];
  const int i = b.blk * kThreads + threadIdx.x;
  if (i >= len) return;
  const float* part = t.ws[b.s] + i;
  float sum = 0.f;
  for (int k = 0; k < slots; ++k) sum += part[(int64_t)k * len];
  t.p[b.s][i] = sum;
}

// ---- Q = M'^T P ----------------------------------------------------------------------
// Slots: g, e, p; q = Q itself (one row tile) or the partial slab [row tiles][m][r].
template <typename T, int RP>
__global__ __launch_bounds__(kThreads) void psgd_backproject_kernel(PsgdTable t) {
  constexpr int CW = kBackCW<RP>, TC = kLanes * CW, TR = kBackRows<RP>, NA = CW * RP;
  __shared__ __attribute__((aligned(16))) float ps[TR][RP];
  __shared__ float red[kRG / 2][NA][kLanes];
  const Seg b = block_seg(t);
  const int n = t.n[b.s], m = t.m[b.s], r = t.r[b.s];
  const int nCT = (m + TC - 1) / TC, rt = b.blk / nCT, ct = b.blk % nCT;
  const T* g = reinterpret_cast<const T*>(t.g[b.s]);
  const float* e = t.e[b.s];
  float* dst = t.q[b.s] + (int64_t)rt * m * r;  // (rt = 0 with one row tile)
  const bool vec = (t.vec >> b.s) & 1;
  fill_rows<TR, RP>(ps, t.p[b.s], (int64_t)rt * TR, n, r);
  __syncthreads();
  const int lane = threadIdx.x % kLanes, rg = threadIdx.x / kLanes;
  const int col0 = ct * TC + lane * CW;
  float acc[CW][RP];
#pragma unroll
  for (int c = 0; c < CW; ++c)
#pragma unroll
    for (int k = 0; k < RP; ++k) acc[c][k] = 0.f;
#pragma unroll 2
  for (int it = 0; it < TR / kRG; ++it) {
    const int lrow = it * kRG + rg, row = rt * TR + lrow;
    float mv[CW];
    ld_m<T, CW>(g, e, (int64_t)row * m + col0, row < n ? m - col0 : 0, vec, mv);
#pragma unroll
    for (int k = 0; k < RP; ++k) {
      const float pk = ps[lrow][k];  // the same address in all 32 lanes of the group
#pragma unroll
      for (int c = 0; c < CW; ++c) acc[c][k] = fmaf(mv[c], pk, acc[c][k]);
    }
  }
  // groups 4..7 onto 0..3, then 2..3 onto 0..1, then 1 onto 0
#pragma unroll
  for (int h = kRG / 2; h >= 1; h >>= 1) {
    if (rg >= h && rg < 2 * h) {
#pragma unroll
      for (int c = 0; c < CW; ++c)
#pragma unroll
        for (int k = 0; k < RP; ++k) red[rg - h][c * RP + k][lane] = acc[c][k];
    }
    __syncthreads();
    if (rg < h) {
#pragma unroll
      for (int c = 0; c < CW; ++c)
#pragma unroll
        for (int k = 0; k < RP; ++k) acc[c][k] += red[rg][c * RP + k][lane];
    }
    __syncthreads();
  }
  if (rg != 0) return;
#pragma unroll
  for (int c = 0; c < CW; ++c)
#pragma unroll
    for (int k = 0; k < RP; ++k)
      if (k < r && col0 + c < m) dst[(int64_t)(col0 + c) * r + k] = acc[c][k];
}

// ---- G <- round(inv_world P Q^T), E <- (G + E) - G_new --------------------------------
// Slots: g, e, p, q
template <typename T, int RP>
__global__ __launch_bounds__(kThreads) void psgd_reconstruct_kernel(PsgdTable t, float inv_world) {
  constexpr int RI = kPR / kRG;  // rows per thread
  __shared__ __attribute__((aligned(16))) float qs[RP][kPC + 4];
  __shared__ __attribute__((aligned(16))) float ps[kPR][RP];
  const Seg b = block_seg(t);
  const int n = t.n[b.s], m = t.m[b.s], r = t.r[b.s];
  const int nCT = (m + kPC - 1) / kPC, rt = b.blk / nCT, ct = b.blk % nCT;
  T* g = reinterpret_cast<T*>(t.g[b.s]);
  float* e = t.e[b.s];
  const bool vec = (t.vec >> b.s) & 1;
  fill_qs<RP>(qs, t.q[b.s], ct, m, r);
  fill_rows<kPR, RP>(ps, t.p[b.s], (int64_t)rt * kPR, n, r);
  __syncthreads();
  const int lane = threadIdx.x % kLanes, rg = threadIdx.x / kLanes;
  const int col0 = ct * kPC + lane * 8;
  float acc[RI][8];
#pragma unroll
  for (int i = 0; i < RI; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
#pragma unroll 4
  for (int k = 0; k < RP; ++k) {
    const dev::f32x4 qa = *reinterpret_cast<const dev::f32x4*>(&qs[k][lane * 8]);
    const dev::f32x4 qb = *reinterpret_cast<const dev::f32x4*>(&qs[k][lane * 8 + 4]);
    const float q8[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
#pragma unroll
    for (int i = 0; i < RI; ++i) {
      const float pk = ps[i * kRG + rg][k];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(pk, q8[j], acc[i][j]);
    }
  }
#pragma unroll
  for (int i = 0; i < RI; ++i) {
    const int row = rt * kPR + i * kRG + rg;
    const int valid = row < n ? m - col0 : 0;
    const int64_t off = (int64_t)row * m + col0;
    float a[8], mv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = inv_world * acc[i][j];
    Vec8<T>::rt(a);  // what the optimizer will read
    if (e) {
      ld_m<T, 8>(g, e, off, valid, vec, mv);
#pragma unroll
      for (int j = 0; j < 8; ++j) mv[j] -= a[j];
      st_cols<float, 8>(e, off, valid, vec, mv);
    }
    st_cols<T, 8>(g, off, valid, vec, a);
  }
}

// ---- CholeskyQR2 ---------------------------------------------------------------------
// Slots of the three kernels: p = X [n, r]; ws = the Gram slots [row blocks][RP][RP], then L^-T [RP][RP].
template <int RP>
__global__ __launch_bounds__(kThreads) void psgd_gram_kernel(PsgdTable t) {
  constexpr int NE = RP * RP, NT = NE < kThreads ? NE : kThreads, EPT = NE / NT, NG = kThreads / NT;
  __shared__ float xs[kOR][RP];
  __shared__ float red[NG][NT];
  const Seg b = block_seg(t);
  const int n = t.n[b.s], r = t.r[b.s];
  fill_rows<kOR, RP>(xs, t.p[b.s], (int64_t)b.blk * kOR, n, r);
  __syncthreads();
  const int rows = min(kOR, n - b.blk * kOR);
  const int e0 = threadIdx.x % NT, grp = threadIdx.x / NT;
  float acc[EPT];
#pragma unroll
  for (int i = 0; i < EPT; ++i) acc[i] = 0.f;
  for (int row = grp; row < rows; row += NG) {
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int e = e0 + i * NT;
      acc[i] = fmaf(xs[row][e / RP], xs[row][e % RP], acc[i]);
    }
  }
  float* out = t.ws[b.s] + (int64_t)b.blk * NE;
  if (NG > 1) {  // (then EPT = 1) the row groups' sums in group order
    red[grp][e0] = acc[0];
    __syncthreads();
    if (threadIdx.x < NT) {
      float sum = 0.f;
      for (int k = 0; k < NG; ++k) sum += red[k][threadIdx.x];
      out[threadIdx.x] = sum;
    }
  } else {
#pragma unroll
    for (int i = 0; i < EPT; ++i) out[e0 + i * NT] = acc[i];
  }
}

// Block s (one wave) is matrix s of the table.
template <int RP>
__global__ __launch_bounds__(64) void psgd_chol_kernel(PsgdTable t, float eps) {
  constexpr int NE = RP * RP;
  __shared__ float a[RP][RP + 1], li[RP][RP + 1];
  __shared__ float reg;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int n = t.n[s], r = t.r[s], nRB = (n + kOR - 1) / kOR;
  const float* gp = t.ws[s];
  float* w = t.ws[s] + (int64_t)nRB * NE;
  for (int e = tid; e < NE; e += 64) {
    double sum = 0.0;
    for (int rb = 0; rb < nRB; ++rb) sum += (double)gp[(int64_t)rb * NE + e];
    a[e / RP][e % RP] = (float)sum;
    li[e / RP][e % RP] = 0.f;
  }
  __syncthreads();
  if (tid == 0) {
    float mx = a[0][0];
    for (int j = 1; j < r; ++j) mx = fmaxf(mx, a[j][j]);
    reg = fmaxf(eps, 0.f) + 1e-10f * mx + 1e-30f;
  }
  __syncthreads();
  if (tid < r) a[tid][tid] += reg;
  __syncthreads();
  for (int k = 0; k < r; ++k) {  // the lower triangle of a becomes L
    if (tid == 0) a[k][k] = sqrtf(a[k][k]);
    __syncthreads();
    if (tid > k && tid < r) a[tid][k] /= a[k][k];
    __syncthreads();
    for (int idx = tid; idx < r * r; idx += 64) {
      const int i = idx / r, j = idx % r;
      if (j > k && i >= j) a[i][j] -= a[i][k] * a[j][k];
    }
    __syncthreads();
  }
  if (tid < r) {  // column tid of L^-1 by forward substitution
    for (int i = tid; i < r; ++i) {
      float sum = i == tid ? 1.f : 0.f;
      for (int j = tid; j < i; ++j) sum -= a[i][j] * li[j][tid];
      li[i][tid] = sum / a[i][i];
    }
  }
  __syncthreads();
  for (int e = tid; e < NE; e += 64) {
    const int j = e / RP, k = e % RP;
    w[e] = (j <= k && k < r) ? li[k][j] : 0.f;  // L^-T, upper triangular
  }
}

template <int RP>
__global__ __launch_bounds__(kThreads) void psgd_apply_kernel(PsgdTable t) {
  __shared__ float w[RP][RP];
  const Seg b = block_seg(t);
  const int n = t.n[b.s], r = t.r[b.s], nRB = (n + kOR - 1) / kOR;
  const float* wsrc = t.ws[b.s] + (int64_t)nRB * RP * RP;
  for (int e = threadIdx.x; e < RP * RP; e += kThreads) w[e / RP][e % RP] = wsrc[e];
  __syncthreads();
  const int64_t row = (int64_t)b.blk * kOR + threadIdx.x;
  if (row >= n) return;
  float* x = t.p[b.s] + row * r;
  float xv[RP];
#pragma unroll
  for (int j = 0; j < RP; ++j) xv[j] = j < r ? x[j] : 0.f;
#pragma unroll
  for (int k = 0; k < RP; ++k) {
    float o = 0.f;
#pragma unroll
    for (int j = 0; j <= k; ++j) o = fmaf(xv[j], w[j][k], o);
    if (k < r) x[k] = o;
  }
}

// ---- host ----------------------------------------------------------------------------
int pad_rank(int r) {
  int p = 1;
  while (p < r) p *= 2;
  return p;
}
int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
int64_t round4(int64_t x) { return (x + 3) / 4 * 4; }

#define PSGD_RANK(rp, ...)                                  \
  switch (rp) {                                             \
    case 1: { constexpr int RP = 1; __VA_ARGS__; break; }   \
    case 2: { constexpr int RP = 2; __VA_ARGS__; break; }   \
    case 4: { constexpr int RP = 4; __VA_ARGS__; break; }   \
    case 8: { constexpr int RP = 8; __VA_ARGS__; break; }   \
    case 16: { constexpr int RP = 16; __VA_ARGS__; break; } \
    case 32: { constexpr int RP = 32; __VA_ARGS__; break; } \
    default: TORCH_CHECK(false, "powersgd: bad padded rank ", rp); \
  }

int back_cols(int rp) { return kLanes * (rp <= 8 ? 8 : 64 / rp); }
int back_rows(int rp) { return rp == 32 ? 128 : 64; }

struct Launch {
  PsgdTable t;
  int blocks;
};

// One segment of a table under construction
struct SegInit {
  void* g = nullptr;
  float *e = nullptr, *p = nullptr, *q = nullptr, *ws = nullptr;
  int n = 0, m = 0, r = 0;
  bool vec = false;
  int64_t blocks = 0;
};

void add_seg(std::vector<Launch>& out, const SegInit& si) {
  if (si.blocks == 0) return;
  TORCH_CHECK(si.blocks < (1ll << 30), "powersgd: matrix too large");
  if (out.empty() || out.back().t.nseg == kMaxSeg || out.back().blocks + si.blocks > (1ll << 30)) {
    out.emplace_back();
    out.back().t.nseg = 0;
    out.back().t.vec = 0;
    out.back().blocks = 0;
  }
  Launch& l = out.back();
  const int s = l.t.nseg++;
  l.t.g[s] = si.g, l.t.e[s] = si.e, l.t.p[s] = si.p, l.t.q[s] = si.q, l.t.ws[s] = si.ws;
  l.t.n[s] = si.n, l.t.m[s] = si.m, l.t.r[s] = si.r;
  if (si.vec) l.t.vec |= 1ull << s;
  l.blocks += (int)si.blocks;
  l.t.blk_end[s] = l.blocks;
}

template <typename K, typename... A>
void run(K kernel, const std::vector<Launch>& ls, int threads, bool per_seg, hipStream_t stream, A... args) {
  for (const Launch& l : ls) {
    hipLaunchKernelGGL(kernel, dim3(per_seg ? l.t.nseg : l.blocks), dim3(threads), 0, stream, l.t, args...);
    XDDP_HIP_CHECK(hipGetLastError());
  }
}

// The tables of CholeskyQR2 over matrices of one padded rank
struct Ortho {
  std::vector<Launch> ls;
  static int64_t ws_floats(int n, int rp) { return round4((cdiv(n, kOR) + 1) * rp * rp); }
  void add(float* x, int n, int r, float* ws) {
    SegInit si;
    si.p = x, si.ws = ws, si.n = n, si.r = r, si.blocks = cdiv(n, kOR);
    add_seg(ls, si);
  }
  void run_all(int rp, float eps, hipStream_t stream) const {
    if (ls.empty()) return;
    PSGD_RANK(rp, {
      for (int pass = 0; pass < 2; ++pass) {
        run(psgd_gram_kernel<RP>, ls, kThreads, false, stream);
        run(psgd_chol_kernel<RP>, ls, 64, true, stream, eps);
        run(psgd_apply_kernel<RP>, ls, kThreads, false, stream);
      }
    });
  }
};

void check_f32(const char* what, const at::Tensor& x, const at::Device& dev) {
  TORCH_CHECK(x.is_cuda() && x.device() == dev && x.scalar_type() == at::kFloat && x.is_contiguous(),
              "powersgd: ", what, " must be a contiguous fp32 tensor on the matrices' device");
}

hipStream_t current_stream(const at::Tensor& x) { return c10::hip::getCurrentHIPStream(x.device().index()).stream(); }

}  // namespace

// The tables of one padded rank
struct RankGroup {
  int rp = 0;
  std::vector<Launch> proj, pfold, back, qfold, recon;
  Ortho op, oq;
};

struct PsgdPlan::Impl {
  std::vector<at::Tensor> keep;
  at::Tensor ws;
  at::ScalarType dtype = at::kFloat;
  std::vector<RankGroup> groups;
  int64_t ws_floats = 0;
};

PsgdPlan::~PsgdPlan() = default;
int64_t PsgdPlan::workspace_floats() const { return impl_->ws_floats; }

PsgdPlan::PsgdPlan(const std::vector<at::Tensor>& mats, const std::vector<at::Tensor>& errors,
                   const std::vector<at::Tensor>& ps, const std::vector<at::Tensor>& qs)
    : impl_(new Impl) {
  const size_t N = mats.size();
  TORCH_CHECK(N > 0, "powersgd: empty matrix list");
  const bool has_e = !errors.empty();
  TORCH_CHECK(ps.size() == N && qs.size() == N && (!has_e || errors.size() == N), "powersgd: list length mismatch");
  Impl& im = *impl_;
  im.dtype = mats[0].scalar_type();
  TORCH_CHECK(im.dtype == at::kFloat || im.dtype == at::kBFloat16 || im.dtype == at::kHalf,
              "powersgd: matrices must be fp32, bf16 or fp16, got ", im.dtype);
  const at::Device dev = mats[0].device();
  struct Geo {
    int n, m, r, rp;
    int64_t o_pp, o_qp, o_op, o_oq;
  };
  std::vector<Geo> geo(N);
  int64_t total = 0;
  for (size_t i = 0; i < N; ++i) {
    const at::Tensor& g = mats[i];
    TORCH_CHECK(g.is_cuda() && g.device() == dev && g.scalar_type() == im.dtype && g.dim() == 2 && g.is_contiguous() &&
                    g.numel() > 0,
                "powersgd: matrices must be non-empty contiguous 2-D device tensors of one dtype");
    const int64_t n = g.size(0), m = g.size(1);
    TORCH_CHECK(n < (1ll << 31) && m < (1ll << 31), "powersgd: dimension too large");
    check_f32("P", ps[i], dev);
    check_f32("Q", qs[i], dev);
    TORCH_CHECK(ps[i].dim() == 2 && qs[i].dim() == 2 && ps[i].size(0) == n && qs[i].size(0) == m &&
                    ps[i].size(1) == qs[i].size(1),
                "powersgd: P must be [n, r] and Q [m, r] for a matrix [n, m]");
    const int64_t r = ps[i].size(1);
    TORCH_CHECK(r >= 1 && r <= kMaxRank && r <= n && r <= m, "powersgd: rank must be in 1..", kMaxRank,
                " and at most min(n, m), got ", r);
    TORCH_CHECK((n + m) * r < (1ll << 31), "powersgd: P or Q too large");
    if (has_e) {
      check_f32("the error memory", errors[i], dev);
      TORCH_CHECK(errors[i].numel() == g.numel(), "powersgd: the error memory must have the matrix's size");
    }
    const int rp = pad_rank((int)r);
    Geo& q = geo[i];
    q = {(int)n, (int)m, (int)r, rp, 0, 0, 0, 0};
    const int64_t nct = cdiv(m, kPC), nrt = cdiv(n, back_rows(rp));
    q.o_pp = total;
    total += nct > 1 ? round4(nct * n * r) : 0;
    q.o_qp = total;
    total += nrt > 1 ? round4(nrt * m * r) : 0;
    q.o_op = total;
    total += Ortho::ws_floats((int)n, rp);
    q.o_oq = total;
    total += Ortho::ws_floats((int)m, rp);
  }
  im.ws_floats = total;
  im.ws = at::empty({total}, at::TensorOptions().dtype(at::kFloat).device(dev));
  float* ws = im.ws.data_ptr<float>();
  for (const auto* list : {&mats, &errors, &ps, &qs}) im.keep.insert(im.keep.end(), list->begin(), list->end());
  for (int rp = 1; rp <= kMaxRank; rp *= 2) {
    RankGroup grp;
    grp.rp = rp;
    for (size_t i = 0; i < N; ++i) {
      const Geo& q = geo[i];
      if (q.rp != rp) continue;
      SegInit si;
      si.g = mats[i].data_ptr();
      si.e = has_e ? errors[i].data_ptr<float>() : nullptr;
      float* p = ps[i].data_ptr<float>();
      float* qq = qs[i].data_ptr<float>();
      si.n = q.n, si.m = q.m, si.r = q.r;
      si.vec = q.m % 8 == 0 && aligned16(si.g) && aligned16(si.e);
      const int64_t nct = cdiv(q.m, kPC), nrt = cdiv(q.n, back_rows(rp));
      // project: the tile sums go to P or to the column-tile slots
      si.q = qq, si.p = nct > 1 ? ws + q.o_pp : p, si.blocks = cdiv(q.n, kPR) * nct;
      add_seg(grp.proj, si);
      if (nct > 1) {
        SegInit f;
        f.p = p, f.ws = ws + q.o_pp, f.n = q.n * q.r, f.m = (int)nct, f.blocks = cdiv((int64_t)q.n * q.r, kThreads);
        add_seg(grp.pfold, f);
      }
      // backproject: to Q or to the row-tile slots
      si.p = p, si.q = nrt > 1 ? ws + q.o_qp : qq, si.blocks = nrt * cdiv(q.m, back_cols(rp));
      add_seg(grp.back, si);
      if (nrt > 1) {
        SegInit f;
        f.p = qq, f.ws = ws + q.o_qp, f.n = q.m * q.r, f.m = (int)nrt, f.blocks = cdiv((int64_t)q.m * q.r, kThreads);
        add_seg(grp.qfold, f);
      }
      si.p = p, si.q = qq, si.blocks = cdiv(q.n, kPR) * nct;
      add_seg(grp.recon, si);
      grp.op.add(p, q.n, q.r, ws + q.o_op);
      grp.oq.add(qq, q.m, q.r, ws + q.o_oq);
    }
    if (!grp.proj.empty()) im.groups.push_back(std::move(grp));
  }
}

void PsgdPlan::project() {
  const hipStream_t stream = current_stream(impl_->ws);
  for (const RankGroup& g : impl_->groups) {
    XDDP_DISPATCH_FLOAT_NO_F64(impl_->dtype, T, "powersgd: unsupported dtype ", {
      PSGD_RANK(g.rp, { run(psgd_project_kernel<T, RP>, g.proj, kThreads, false, stream); });
    });
    run(psgd_fold_kernel, g.pfold, kThreads, false, stream);
  }
}

void PsgdPlan::backproject() {
  const hipStream_t stream = current_stream(impl_->ws);
  for (const RankGroup& g : impl_->groups) {
    XDDP_DISPATCH_FLOAT_NO_F64(impl_->dtype, T, "powersgd: unsupported dtype ", {
      PSGD_RANK(g.rp, { run(psgd_backproject_kernel<T, RP>, g.back, kThreads, false, stream); });
    });
    run(psgd_fold_kernel, g.qfold, kThreads, false, stream);
  }
}

void PsgdPlan::reconstruct(double inv_world) {
  const hipStream_t stream = current_stream(impl_->ws);
  for (const RankGroup& g : impl_->groups) {
    XDDP_DISPATCH_FLOAT_NO_F64(impl_->dtype, T, "powersgd: unsupported dtype ", {
      PSGD_RANK(g.rp, { run(psgd_reconstruct_kernel<T, RP>, g.recon, kThreads, false, stream, (float)inv_world); });
    });
  }
}

void PsgdPlan::orthonormalize_p(double epsilon) {
  for (const RankGroup& g : impl_->groups) g.op.run_all(g.rp, (float)epsilon, current_stream(impl_->ws));
}
void PsgdPlan::orthonormalize_q(double epsilon) {
  for (const RankGroup& g : impl_->groups) g.oq.run_all(g.rp, (float)epsilon, current_stream(impl_->ws));
}

void psgd_orthonormalize(const std::vector<at::Tensor>& mats, double epsilon) {
  TORCH_CHECK(!mats.empty(), "powersgd: empty matrix list");
  const at::Device dev = mats[0].device();
  std::vector<int64_t> off(mats.size());
  int64_t total = 0;
  for (size_t i = 0; i < mats.size(); ++i) {
    const at::Tensor& x = mats[i];
    check_f32("a matrix to orthonormalize", x, dev);
    TORCH_CHECK(x.dim() == 2 && x.size(1) >= 1 && x.size(1) <= kMaxRank && x.size(1) <= x.size(0) &&
                    x.numel() < (1ll << 31),
                "powersgd: orthonormalize takes [n, r] matrices with 1 <= r <= min(n, ", kMaxRank, ")");
    off[i] = total;
    total += Ortho::ws_floats((int)x.size(0), pad_rank((int)x.size(1)));
  }
  at::Tensor ws = at::empty({total}, at::TensorOptions().dtype(at::kFloat).device(dev));
  const hipStream_t stream = current_stream(ws);
  for (int rp = 1; rp <= kMaxRank; rp *= 2) {
    Ortho o;
    for (size_t i = 0; i < mats.size(); ++i)
      if (pad_rank((int)mats[i].size(1)) == rp)
        o.add(mats[i].data_ptr<float>(), (int)mats[i].size(0), (int)mats[i].size(1), ws.data_ptr<float>() + off[i]);
    o.run_all(rp, (float)epsilon, stream);
  }
}

}  // namespace kernels
}  // namespace xddp
