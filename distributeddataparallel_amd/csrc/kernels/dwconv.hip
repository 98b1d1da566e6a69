// Depthwise k x k convolution (k in {3, 5, 7}, stride 1, padding k / 2, groups == C) on NHWC
// tensors x [B, C, H, W] channels_last (bf16 / fp16 / fp32, C % 8 == 0, 16-B aligned base): the
// forward, the input gradient (the same kernel on dy with the taps flipped) and the weight + bias
// gradient. fp32 accumulation, one rounding to the output dtype. MFMA does not fit (nothing is
// reduced across channels), so this is a vector-FMA kernel whose whole point is register reuse: at
// k = 7 an input value takes part in 49 FMAs, and LDS could not feed one read per FMA.
//
// Tiling. A block of 256 threads owns a slab of 64 bytes of channels (32 of a 16-bit type, 16 of
// fp32: the ConvNeXt widths 96 .. 768 split into whole slabs) and 16 patches of 4 x 4 output
// pixels: one image's 16 x 16 tile (4 x 4 patches), or, for maps of at most 8 x 8, the 8 x 8 tiles
// of four images (2 x 2 patches each), so that a 7 x 7 map at C = 768 still fills the block. A
// thread owns one 32-bit word of channels (2 of a 16-bit type, 1 of fp32: lane & 15 picks the
// word, so 16 lanes read one pixel's 64 B) and one patch (thread >> 4; a wave holds four patches
// that are neighbours along x).
//
// Staging. The block copies each image's halo tile ((4 TPY + k - 1) x (4 TPX + k - 1) pixels of the
// slab) to LDS with 16-B loads, with zeros for the padding, for pixels past the map or the batch
// and for channels past C: the tap loops have no bounds test. LDS keeps the storage dtype (half
// the bytes, and the unpack is 2 VALU operations per 2 x 16 FMAs). A pixel is 16 words; column c of
// a row sits at slot c + c / 4, so that the four patches of a wave (4 columns apart) start 5, 10,
// 15 slots apart: they read from four different 16-word bank groups, where unpadded they would all
// hit the same one. A thread's column is 4 px + u, so its slot is 5 px + (u + u / 4): a per-thread
// base plus a compile-time offset.
//
// Registers. Forward: the thread's k x k taps per channel live in registers (flipped on load for
// the input gradient: tap t reads w[k k - 1 - t], no second kernel and no flipped copy), with 4 x 4
// accumulators per channel. It walks the 4 + k - 1 halo rows of its patch; of each it reads the
// 4 + k - 1 words once and uses every value in up to 4 (output rows) x k (taps of that row)
// FMAs per channel: 100 LDS reads for 784 FMAs per channel at k = 7. Weight gradient: the roles
// swap: the thread's 4 x 4 dy values per channel live in registers, the accumulators are the
// k x k taps (+ 1 for the bias), and the same halo walk feeds them. Everything is unrolled, so every
// register array has constant indices.
//
// Weight gradient reduction (no float atomics, no host synchronisation: bitwise repeatable, equal
// on every replica). A block walks tiles g, g + G, g + 2 G, ... of its slab with its accumulators
// in registers; then the 16 threads that share a channel word fold through LDS in patch order,
// 25 values per thread at a time, and the block writes its partial to its own slot
// part[g][k k + 1][C] (fp32). dwconv_fold_kernel adds the G slots in order and writes dw in the
// weight's [C, 1, k, k] layout and dtype, and db. The workspace comes from torch's caching
// allocator; all launches go to the current stream and can be captured in a graph.
//
// The file is built without packed fp32 operations (_build.EXTRA_HIP_FLAGS) like the other files
// that promise equal bits on every replica.
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include "common.h"
#include "kernels/dev_utils.h"
#include "kernels/norm.h"

namespace xddp {
namespace kernels {

namespace {

constexpr int kDT = 256;     // threads per block
constexpr int kDP = 4;       // patch edge (output pixels)
constexpr int kDPatches = 16;  // patches per block
constexpr int kDWords = 16;  // 32-bit words of channels per slab (64 B per pixel)
constexpr int kDFold = 25;   // accumulators per thread that go through LDS at a time

// one 32-bit word of channels in compute type
template <typename T>
struct Word;
template <>
struct Word<dev::bf16_t> {
  static constexpr int kC = 2;
  static __device__ __forceinline__ void unpack(uint32_t d, float (&f)[2]) {
    f[0] = __uint_as_float(d << 16);
    f[1] = __uint_as_float(d & 0xffff0000u);
  }
  static __device__ __forceinline__ uint32_t pack(const float (&f)[2]) { return dev::pack_bf16x2(f[0], f[1]); }
};
template <>
struct Word<dev::f16_t> {
  static constexpr int kC = 2;
  static __device__ __forceinline__ void unpack(uint32_t d, float (&f)[2]) {
    f[0] = dev::f16_to_f32((uint16_t)(d & 0xffffu));
    f[1] = dev::f16_to_f32((uint16_t)(d >> 16));
  }
  static __device__ __forceinline__ uint32_t pack(const float (&f)[2]) { return dev::pack_f16x2(f[0], f[1]); }
};
template <>
struct Word<float> {
  static constexpr int kC = 1;
  static __device__ __forceinline__ void unpack(uint32_t d, float (&f)[1]) { f[0] = __uint_as_float(d); }
  static __device__ __forceinline__ uint32_t pack(const float (&f)[1]) { return __float_as_uint(f[0]); }
};

// slot of column c in an LDS row (see "Staging"), and the slots a row of n columns takes
__host__ __device__ constexpr int col_slot(int c) { return c + c / 4; }
__host__ __device__ constexpr int row_slots(int n) { return col_slot(n - 1) + 1; }

struct Geo {
  int B, C, H, W;
  int tpy, tpx, imgs;    // patches per image tile along y and x, images per block (imgs tpy tpx = 16)
  int tiles_y, tiles_x;  // tiles per image
  int ntiles;            // image groups x tiles_y x tiles_x
  int slabs;
};

struct Tile {
  int n0, y0, x0;  // first image, origin of the output tile
};

__device__ __forceinline__ Tile tile_of(const Geo& g, int t) {
  Tile r;
  r.x0 = (t % g.tiles_x) * g.tpx * kDP;
  t /= g.tiles_x;
  r.y0 = (t % g.tiles_y) * g.tpy * kDP;
  r.n0 = (t / g.tiles_y) * g.imgs;
  return r;
}

// Copies, for each of the block's images, the rows x cols pixels of the slab that starts at channel
// c0 and whose first pixel is (y0 - pad, x0 - pad) to lds, 16 B per item, zeros where the source
// does not exist. Image i's region starts at slot i rows rsp.
template <typename T>
__device__ __forceinline__ void stage(const T* __restrict__ src, uint32_t* lds, const Geo& g, const Tile& t, int c0,
                                      int pad, int rows, int cols) {
  constexpr int kPer16 = 16 / (int)sizeof(T);
  const int rsp = row_slots(cols);
  const int items = g.imgs * rows * cols * 4;
  for (int e = threadIdx.x; e < items; e += kDT) {
    const int q = e & 3;
    int p = e >> 2;
    const int c = p % cols;
    p /= cols;
    const int r = p % rows, i = p / rows;
    const int n = t.n0 + i, y = t.y0 + r - pad, x = t.x0 + c - pad, ch = c0 + q * kPer16;
    dev::u32x4 v = {0u, 0u, 0u, 0u};
    if (n < g.B && y >= 0 && y < g.H && x >= 0 && x < g.W && ch < g.C)
      v = *reinterpret_cast<const dev::u32x4*>(src + (((int64_t)n * g.H + y) * g.W + x) * g.C + ch);
    *reinterpret_cast<dev::u32x4*>(lds + ((i * rows + r) * rsp + col_slot(c)) * kDWords + q * 4) = v;
  }
}

// the thread's patch: image i of the block, patch row py and column px of its tile
struct Patch {
  int i, py, px;
};
__device__ __forceinline__ Patch patch_of(const Geo& g) {
  int s = threadIdx.x >> 4;
  Patch p;
  p.px = s % g.tpx;
  s /= g.tpx;
  p.py = s % g.tpy;
  p.i = s / g.tpy;
  return p;
}

// The halo walk keeps one row ahead: a row's words are read (raw) while the row before it is in the
// FMAs, and a scheduling barrier after each row keeps the compiler from hoisting every row's reads
// to the top, which costs more registers than the k = 7 kernels have at two waves per SIMD.
template <int R>
__device__ __forceinline__ void load_row(uint32_t (&raw)[R], const uint32_t* row) {
#pragma unroll
  for (int u = 0; u < R; ++u) raw[u] = row[col_slot(u) * kDWords];
}
// in = the row held in raw, in compute type; then raw = the row at `next` (if there is one)
template <typename T, int R>
__device__ __forceinline__ void next_row(float (&in)[Word<T>::kC][R], uint32_t (&raw)[R], const uint32_t* next,
                                         bool more) {
#pragma unroll
  for (int u = 0; u < R; ++u) {
    float f[Word<T>::kC];
    Word<T>::unpack(raw[u], f);
#pragma unroll
    for (int c = 0; c < Word<T>::kC; ++c) in[c][u] = f[c];
  }
  if (more) load_row<R>(raw, next);
}

// y = conv(x, w) + bias; flip: the taps in reverse order (the input gradient, src = dy). wt is tap-major
// [K K, C].
template <typename T, int K>
__global__ __launch_bounds__(kDT, 2) void dwconv_fwd_kernel(const T* __restrict__ src, const T* __restrict__ wt,
                                                         const T* __restrict__ bias, T* __restrict__ out, Geo g,
                                                         int flip) {
  using Wd = Word<T>;
  constexpr int CP = Wd::kC, KK = K * K, R = kDP + K - 1;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int slab = blockIdx.x % g.slabs;
  const Tile t = tile_of(g, blockIdx.x / g.slabs);
  const int c0 = slab * kDWords * CP;
  const int rows = g.tpy * kDP + K - 1, cols = g.tpx * kDP + K - 1;
  stage<T>(src, lds, g, t, c0, K / 2, rows, cols);

  const int cw = threadIdx.x & 15;
  const int ch = c0 + cw * CP;  // C % CP == 0: the word's channels exist together
  const bool live = ch < g.C;
  // the word's taps, one 32-bit load per tap (tap-major: the word's channels are neighbours); a
  // scheduling barrier per tap row keeps the addresses of at most K loads alive at a time
  const uint32_t* ww = reinterpret_cast<const uint32_t*>(wt) + (live ? ch / CP : 0);
  // (a start and a signed step, not a select per tap: the compiler turns "flip ? w[KK - 1 - k] : w[k]" into
  // both sets of registers and a select at every use)
  const int wstep = flip ? -(g.C / CP) : g.C / CP, wstart = flip ? (KK - 1) * (g.C / CP) : 0;
  float w[CP][KK];
#pragma unroll
  for (int k = 0; k < KK; ++k) {
    float f[CP];
    Wd::unpack(ww[wstart + k * wstep], f);
#pragma unroll
    for (int c = 0; c < CP; ++c) w[c][k] = f[c];
    if (k % K == K - 1) __builtin_amdgcn_sched_barrier(0);
  }
  float acc[CP][kDP][kDP];
  {
    float b[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) b[c] = 0.f;
    if (bias != nullptr && live) Wd::unpack(reinterpret_cast<const uint32_t*>(bias)[ch / CP], b);
#pragma unroll
    for (int c = 0; c < CP; ++c)
#pragma unroll
      for (int a = 0; a < kDP * kDP; ++a) acc[c][a / kDP][a % kDP] = b[c];
  }
  const Patch p = patch_of(g);
  const int rsp = row_slots(cols);
  const uint32_t* base = lds + ((p.i * rows + p.py * kDP) * rsp + 5 * p.px) * kDWords + cw;
  __syncthreads();

  uint32_t raw[R];
  load_row<R>(raw, base);
#pragma unroll
  for (int v = 0; v < R; ++v) {
    float in[CP][R];
    next_row<T, R>(in, raw, base + (v + 1) * rsp * kDWords, v + 1 < R);
#pragma unroll
    for (int oy = 0; oy < kDP; ++oy) {
      const int i = v - oy;  // tap row that joins halo row v to output row oy
      if (i < 0 || i >= K) continue;
#pragma unroll
      for (int j = 0; j < K; ++j)
#pragma unroll
        for (int ox = 0; ox < kDP; ++ox)
#pragma unroll
          for (int c = 0; c < CP; ++c) acc[c][oy][ox] = fmaf(in[c][ox + j], w[c][i * K + j], acc[c][oy][ox]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }

  // The sums are complete here, whatever becomes of them: without this the compiler sinks each
  // pixel's FMA chain into that pixel's "inside the map" branch below, which keeps the whole halo
  // patch in registers at once.
#pragma unroll
  for (int c = 0; c < CP; ++c)
#pragma unroll
    for (int a = 0; a < kDP * kDP; ++a) asm volatile("" : "+v"(acc[c][a / kDP][a % kDP]));

  const int n = t.n0 + p.i;
  if (!live || n >= g.B) return;
  uint32_t* o = reinterpret_cast<uint32_t*>(out);
#pragma unroll
  for (int oy = 0; oy < kDP; ++oy) {
    const int y = t.y0 + p.py * kDP + oy;
    if (y >= g.H) break;
#pragma unroll
    for (int ox = 0; ox < kDP; ++ox) {
      const int x = t.x0 + p.px * kDP + ox;
      if (x >= g.W) break;
      float f[CP];
#pragma unroll
      for (int c = 0; c < CP; ++c) f[c] = acc[c][oy][ox];
      o[((((int64_t)n * g.H + y) * g.W + x) * g.C + ch) / CP] = Wd::pack(f);
    }
  }
}

// part[blockIdx.y][t][ch] = sum over the block's tiles of dy[b, y, x, ch] x[b, y + i - p, x + j - p, ch]
// (t = i K + j), and of dy alone at t = K K.
template <typename T, int K>
__global__ __launch_bounds__(kDT, 2) void dwconv_wgrad_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                           float* __restrict__ part, Geo g) {
  using Wd = Word<T>;
  constexpr int CP = Wd::kC, KK = K * K, R = kDP + K - 1, NV = CP * (KK + 1);
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int slab = blockIdx.x, c0 = slab * kDWords * CP;
  const int rows = g.tpy * kDP + K - 1, cols = g.tpx * kDP + K - 1;
  const int drows = g.tpy * kDP, dcols = g.tpx * kDP;
  const int rsp = row_slots(cols), drsp = row_slots(dcols);
  uint32_t* ldy = lds + g.imgs * rows * rsp * kDWords;
  const int cw = threadIdx.x & 15;
  const Patch p = patch_of(g);
  const uint32_t* xb = lds + ((p.i * rows + p.py * kDP) * rsp + 5 * p.px) * kDWords + cw;
  const uint32_t* db = ldy + ((p.i * drows + p.py * kDP) * drsp + 5 * p.px) * kDWords + cw;

  float acc[CP][KK + 1];
#pragma unroll
  for (int c = 0; c < CP; ++c)
#pragma unroll
    for (int k = 0; k <= KK; ++k) acc[c][k] = 0.f;

  for (int ti = blockIdx.y; ti < g.ntiles; ti += gridDim.y) {
    const Tile t = tile_of(g, ti);
    __syncthreads();  // the previous tile's reads are done
    stage<T>(x, lds, g, t, c0, K / 2, rows, cols);
    stage<T>(dy, ldy, g, t, c0, 0, drows, dcols);
    __syncthreads();
    float d[CP][kDP][kDP];
#pragma unroll
    for (int oy = 0; oy < kDP; ++oy)
#pragma unroll
      for (int ox = 0; ox < kDP; ++ox) {
        float f[CP];
        Wd::unpack(db[(oy * drsp + col_slot(ox)) * kDWords], f);
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          d[c][oy][ox] = f[c];
          acc[c][KK] += f[c];
        }
      }
    uint32_t raw[R];
    load_row<R>(raw, xb);
#pragma unroll
    for (int v = 0; v < R; ++v) {
      float in[CP][R];
      next_row<T, R>(in, raw, xb + (v + 1) * rsp * kDWords, v + 1 < R);
#pragma unroll
      for (int oy = 0; oy < kDP; ++oy) {
        const int i = v - oy;
        if (i < 0 || i >= K) continue;
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
          for (int ox = 0; ox < kDP; ++ox)
#pragma unroll
            for (int c = 0; c < CP; ++c) acc[c][i * K + j] = fmaf(d[c][oy][ox], in[c][ox + j], acc[c][i * K + j]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // fold the 16 patches of each channel word in patch order, kDFold values per thread at a time
  float* red = reinterpret_cast<float*>(lds);
  const int s = threadIdx.x >> 4;
#pragma unroll
  for (int q0 = 0; q0 < NV; q0 += kDFold) {
    __syncthreads();
#pragma unroll
    for (int ql = 0; ql < kDFold; ++ql)
      if (q0 + ql < NV) red[(s * kDFold + ql) * kDWords + cw] = acc[(q0 + ql) / (KK + 1)][(q0 + ql) % (KK + 1)];
    __syncthreads();
    for (int e = threadIdx.x; e < kDFold * kDWords; e += kDT) {
      const int ql = e >> 4, q = q0 + ql, w = e & 15;
      const int ch = c0 + w * CP + q / (KK + 1);
      if (q >= NV || ch >= g.C) continue;
      float sum = 0.f;
#pragma unroll
      for (int k = 0; k < kDPatches; ++k) sum += red[(k * kDFold + ql) * kDWords + w];
      part[((int64_t)blockIdx.y * (KK + 1) + q % (KK + 1)) * g.C + ch] = sum;
    }
  }
}

// dw[ch][t] = sum over the G slots, in order; db[ch] from row K K
template <typename T>
__global__ __launch_bounds__(kDT) void dwconv_fold_kernel(const float* __restrict__ part, T* __restrict__ dw,
                                                          T* __restrict__ db, int G, int KK, int C) {
  const int e = blockIdx.x * kDT + threadIdx.x;
  if (e >= (KK + 1) * C) return;
  const int t = e / C, ch = e - t * C;
  float sum = 0.f;
  for (int k = 0; k < G; ++k) sum += part[(int64_t)k * (KK + 1) * C + e];
  if (t < KK) dev::Elem<T, float>::st(dw, (int64_t)ch * KK + t, sum);
  else if (db != nullptr) dev::Elem<T, float>::st(db, ch, sum);
}

Geo make_geo(const at::Tensor& x, int cp) {
  Geo g;
  g.B = (int)x.size(0), g.C = (int)x.size(1), g.H = (int)x.size(2), g.W = (int)x.size(3);
  const bool small = g.H <= 2 * kDP && g.W <= 2 * kDP;
  g.tpy = g.tpx = small ? 2 : 4;
  g.imgs = kDPatches / (g.tpy * g.tpx);
  g.tiles_y = (g.H + g.tpy * kDP - 1) / (g.tpy * kDP);
  g.tiles_x = (g.W + g.tpx * kDP - 1) / (g.tpx * kDP);
  g.slabs = (g.C + kDWords * cp - 1) / (kDWords * cp);
  const int64_t ntiles = (int64_t)((g.B + g.imgs - 1) / g.imgs) * g.tiles_y * g.tiles_x;
  TORCH_CHECK(ntiles * g.slabs < (int64_t(1) << 31), "dwconv: too many tiles");
  g.ntiles = (int)ntiles;
  return g;
}

size_t halo_bytes(const Geo& g, int K) {
  return (size_t)g.imgs * (g.tpy * kDP + K - 1) * row_slots(g.tpx * kDP + K - 1) * kDWords * 4;
}

int kernel_size(int64_t taps) { return taps == 9 ? 3 : taps == 25 ? 5 : taps == 49 ? 7 : 0; }

void check_input(const char* what, const at::Tensor& x) {
  const auto st = x.scalar_type();
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && (st == at::kFloat || st == at::kBFloat16 || st == at::kHalf), what,
              " must be a 4-D fp32 / bf16 / fp16 CUDA tensor [B, C, H, W]");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast) && x.size(1) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              what, " must be dense channels_last with C % 8 == 0 and a 16-byte aligned base");
  TORCH_CHECK(x.size(0) < (1 << 30) && x.size(2) < (1 << 24) && x.size(3) < (1 << 24) && x.size(1) < (1 << 24),
              what, ": dimension too large");
}

template <typename T, int K>
void launch_fwd(const at::Tensor& x, const at::Tensor& wt, const T* bias, at::Tensor& y, bool flip,
                hipStream_t stream) {
  const Geo g = make_geo(x, Word<T>::kC);
  const size_t lds = halo_bytes(g, K);
  ensure_dyn_lds((const void*)dwconv_fwd_kernel<T, K>, lds);
  hipLaunchKernelGGL((dwconv_fwd_kernel<T, K>), dim3((unsigned)(g.ntiles * g.slabs)), dim3(kDT), lds, stream,
                     reinterpret_cast<const T*>(x.data_ptr()), reinterpret_cast<const T*>(wt.data_ptr()), bias,
                     reinterpret_cast<T*>(y.data_ptr()), g, flip ? 1 : 0);
}

template <typename T>
void dispatch_fwd(int K, const at::Tensor& x, const at::Tensor& wt, const c10::optional<at::Tensor>& bias,
                  at::Tensor& y, bool flip, hipStream_t stream) {
  const T* b = bias.has_value() ? reinterpret_cast<const T*>(bias->data_ptr()) : nullptr;
  if (K == 3) launch_fwd<T, 3>(x, wt, b, y, flip, stream);
  else if (K == 5) launch_fwd<T, 5>(x, wt, b, y, flip, stream);
  else launch_fwd<T, 7>(x, wt, b, y, flip, stream);
}

template <typename T, int K>
void launch_wgrad(const at::Tensor& dy, const at::Tensor& x, at::Tensor& dw, at::Tensor* db, hipStream_t stream) {
  const Geo g = make_geo(x, Word<T>::kC);
  constexpr int KK = K * K;
  // about three blocks per CU over all slabs; each walks ntiles / G tiles with its sums in registers
  const int G = std::max(1, std::min(g.ntiles, std::min(65535, 768 / g.slabs)));
  auto part = at::empty({G, KK + 1, g.C}, x.options().dtype(at::kFloat));
  const size_t stage_bytes = halo_bytes(g, K) + (size_t)g.imgs * g.tpy * kDP * row_slots(g.tpx * kDP) * kDWords * 4;
  const size_t lds = std::max(stage_bytes, (size_t)kDT * kDFold * 4);
  ensure_dyn_lds((const void*)dwconv_wgrad_kernel<T, K>, lds);
  hipLaunchKernelGGL((dwconv_wgrad_kernel<T, K>), dim3((unsigned)g.slabs, (unsigned)G), dim3(kDT), lds, stream,
                     reinterpret_cast<const T*>(dy.data_ptr()), reinterpret_cast<const T*>(x.data_ptr()),
                     part.data_ptr<float>(), g);
  const int n = (KK + 1) * g.C;
  hipLaunchKernelGGL((dwconv_fold_kernel<T>), dim3((unsigned)((n + kDT - 1) / kDT)), dim3(kDT), 0, stream,
                     part.data_ptr<float>(), reinterpret_cast<T*>(dw.data_ptr()),
                     db != nullptr ? reinterpret_cast<T*>(db->data_ptr()) : nullptr, G, KK, g.C);
}

template <typename T>
void dispatch_wgrad(int K, const at::Tensor& dy, const at::Tensor& x, at::Tensor& dw, at::Tensor* db,
                    hipStream_t stream) {
  if (K == 3) launch_wgrad<T, 3>(dy, x, dw, db, stream);
  else if (K == 5) launch_wgrad<T, 5>(dy, x, dw, db, stream);
  else launch_wgrad<T, 7>(dy, x, dw, db, stream);
}

}  // namespace

at::Tensor dwconv_forward(const at::Tensor& x, const at::Tensor& w_taps, const c10::optional<at::Tensor>& bias,
                          bool flip) {
  check_input("dwconv_forward: x", x);
  const int64_t C = x.size(1);
  const int K = w_taps.dim() == 2 ? kernel_size(w_taps.size(0)) : 0;
  TORCH_CHECK(K != 0 && w_taps.size(1) == C && w_taps.is_contiguous() && w_taps.device() == x.device() &&
                  w_taps.scalar_type() == x.scalar_type(),
              "dwconv_forward: w_taps must be tap-major [k * k, C] (k in 3, 5, 7), contiguous, of x's dtype and device");
  if (bias.has_value())
    TORCH_CHECK(bias->dim() == 1 && bias->size(0) == C && bias->is_contiguous() && bias->device() == x.device() &&
                    bias->scalar_type() == x.scalar_type(),
                "dwconv_forward: bias must be [C], contiguous, of x's dtype and device");
  auto y = at::empty_like(x);  // dense channels_last: the same strides
  if (x.numel() == 0) return y;
  auto stream = c10::hip::getCurrentHIPStream(x.device().index()).stream();
  const auto st = x.scalar_type();
  if (st == at::kFloat) dispatch_fwd<float>(K, x, w_taps, bias, y, flip, stream);
  else if (st == at::kBFloat16) dispatch_fwd<dev::bf16_t>(K, x, w_taps, bias, y, flip, stream);
  else dispatch_fwd<dev::f16_t>(K, x, w_taps, bias, y, flip, stream);
  XDDP_HIP_CHECK(hipGetLastError());
  return y;
}

std::vector<at::Tensor> dwconv_wgrad(const at::Tensor& dy, const at::Tensor& x, int64_t k, bool need_bias) {
  check_input("dwconv_wgrad: x", x);
  check_input("dwconv_wgrad: dy", dy);
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.scalar_type() == x.scalar_type() && dy.device() == x.device(),
              "dwconv_wgrad: dy must have x's shape, dtype and device");
  TORCH_CHECK(k == 3 || k == 5 || k == 7, "dwconv_wgrad: k must be 3, 5 or 7");
  const int64_t C = x.size(1);
  auto dw = at::empty({C, 1, k, k}, x.options());
  at::Tensor db;
  if (need_bias) db = at::empty({C}, x.options());
  if (x.numel() == 0) {
    dw.zero_();
    if (need_bias) db.zero_();
    return {dw, db};
  }
  auto stream = c10::hip::getCurrentHIPStream(x.device().index()).stream();
  const auto st = x.scalar_type();
  at::Tensor* dbp = need_bias ? &db : nullptr;
  if (st == at::kFloat) dispatch_wgrad<float>((int)k, dy, x, dw, dbp, stream);
  else if (st == at::kBFloat16) dispatch_wgrad<dev::bf16_t>((int)k, dy, x, dw, dbp, stream);
  else dispatch_wgrad<dev::f16_t>((int)k, dy, x, dw, dbp, stream);
  XDDP_HIP_CHECK(hipGetLastError());
  return {dw, db};
}

}  // namespace kernels
}  // namespace xddp
