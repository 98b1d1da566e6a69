// Top-k sparsified gradient wire with error feedback: compress, decode-and-average,
// reduce-and-reselect.
//
// Format. A bucket of n elements is cut into blocks of G consecutive elements (G = 1024 | 2048 |
// 4096, the last block may be short) and every block keeps exactly k = 8 | 16 | 32 | 64 entries.
// For a block with c >= 1 real elements x_i and an fp32 residual e_i:
//
//   v_i   = float(x_i) + e_i
//   key_i = bits(|v_i|)                 (uint32, monotone in |v_i|; +0 and -0 tie)
//   the k real elements of largest key are selected, ties going to the lower index
//   slot j (j = 0 .. k-1, ascending index): uint16 offset in the block, fp32 v itself
//   e_i  <- 0 on selected elements, v_i on the others
//
// With c < k the trailing k - c slots are empty: offset 0xFFFF, value 0. A block whose v holds a
// NaN or an inf stores offset 0xFFFF and value NaN in all k slots and leaves its e_i as they were:
// it decodes to NaN on every rank, and one skipped step does not poison the residual.
//
// Payload: S segments of cb blocks; a segment is cb·k fp32 values, then cb·k uint16 offsets
// (6 k / G bytes per element). Padding blocks hold empty slots.
//
// Work split, shared by the three kernels: one wave owns one block, lane l holds the E = G / 64
// consecutive elements [l·E, (l + 1)·E) as keys in registers plus one sign bit each, so index order
// is lane order, then register order.
//
// Selection. T, the k-th largest key, is found exactly by a search over the key's 31 bits from the
// top: a bit stays set while at least k keys are >= the candidate. The count is one v_cmp per
// register whose 64-bit lane mask goes through s_bcnt1 into a scalar sum, so it is wave-uniform
// without a butterfly, and the search stops as soon as a candidate splits off exactly k keys.
// Padding has key 0 and no candidate is 0, so it is never counted.
//
// Compaction. Keys > T are all taken, keys == T from the lowest index until k are. A lane counts
// its two classes, one wave scan of the packed pair gives the classes' counts in the lanes before
// it, and so the slot of its first selected element; it then walks its registers in order. Slots
// are staged in LDS (8 bytes each) and leave as one coalesced store of k values and k offsets: no
// atomics, no sort, ascending by construction. No register array is indexed dynamically.
//
// Decode. A wave zeroes G floats of LDS, then for each of the W versions in order lanes < k store
// (first version) or add (later ones) their slot at its offset: offsets within one version are
// distinct and the versions are separated by a wave-level fence, so the sum is
// ((d_0 + d_1) + ...) + d_{W-1} on every rank. A coalesced pass divides by W (W > 1), converts and
// stores 16 bytes per lane. Reduce-and-reselect scatters the same way into a layout padded by 16
// bytes per lane run, so that every lane reads its E consecutive sums back with conflict-free
// 16-byte LDS reads, adds the server residual and runs the selection above.
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <algorithm>

#include "common.h"
#include "kernels/dev_utils.h"
#include "kernels/lane_vec.h"
#include "kernels/topk_comm.h"

namespace xddp {
namespace kernels {

namespace {

constexpr int kTGroupsPerCU = 8;
constexpr int kTCompressWaves = 4;  // compress holds no block in LDS: 256 threads as the siblings
constexpr uint32_t kAbs = 0x7fffffffu, kInf = 0x7f800000u, kQuietNaN = 0x7fc00000u;
constexpr uint32_t kEmpty = 0xffffu;  // the offset of a slot that holds no element

using dev::LaneVec;

// waves (= blocks in LDS) per workgroup of the kernels that hold a block in LDS: 32 KiB at most
template <int G>
constexpr int lds_waves() { return G == 4096 ? 2 : 4; }

// orders the LDS accesses of the wave's lanes: what a lane wrote before is visible to all after
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One segment's view of block b: its k values and its k offsets.
struct Slots {
  float* val;
  uint16_t* off;
  __device__ __forceinline__ Slots(uint8_t* seg, unsigned cb, unsigned b, int k)
      : val(reinterpret_cast<float*>(seg) + (int64_t)b * k),
        off(reinterpret_cast<uint16_t*>(seg + (int64_t)cb * k * 4) + (int64_t)b * k) {}
  // slots [from, k) hold no element: value 0 (padding) or NaN (a skipped block)
  __device__ __forceinline__ void fill(int lane, int k, int from, uint32_t bits) const {
    if (lane >= from && lane < k) {
      val[lane] = __uint_as_float(bits);
      off[lane] = (uint16_t)kEmpty;
    }
  }
};

// The block as the selection sees it: keys and signs of the lane's E values.
template <int E>
struct Keys {
  uint32_t key[E];
  uint32_t neg[(E + 31) / 32];
  __device__ __forceinline__ void set(const float (&v)[E]) {
#pragma unroll
    for (int w = 0; w < (E + 31) / 32; ++w) neg[w] = 0u;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const uint32_t u = __float_as_uint(v[j]);
      key[j] = u & kAbs;
      neg[j >> 5] |= (u >> 31) << (j & 31);
    }
  }
  __device__ __forceinline__ uint32_t bits(int j) const { return key[j] | (neg[j >> 5] >> (j & 31) & 1u) << 31; }
};

// Select and store the k largest of the block the wave holds (lane: `cl` real elements first, keys 0
// after them; c real elements in the block) into s, and write e <- 0 / v to err[0 .. E) (`vec`: all
// E at once). `stage` is the wave's 64 LDS slots. Every lane of the wave calls this.
template <int G>
__device__ __forceinline__ void select_block(Keys<G / 64>& q, int cl, int k, float* err, bool vec, const Slots& s,
                                             uint2* stage, int lane) {
  constexpr int E = G / 64;
  uint32_t top = 0u;
#pragma unroll
  for (int j = 0; j < E; ++j) top = max(top, q.key[j]);
  if (__ballot(top >= kInf) != 0ull) {  // the residual of a skipped block stays as it was
    s.fill(lane, k, 0, kQuietNaN);
    return;
  }
  // T: the largest value with at least k keys >= T, or, once exactly k keys are >= a candidate,
  // that candidate - 1 (the same set is then "key > T" and no tie is needed); 0 if fewer than k
  // keys are non-zero
  uint32_t T = 0u;
#pragma nounroll
  for (int bit = 30; bit >= 0; --bit) {
    const uint32_t cand = T | 1u << bit;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < E; ++j) cnt += __popcll(__ballot(q.key[j] >= cand));
    if (cnt == k) {
      T = cand - 1u;
      break;
    }
    if (cnt > k) T = cand;
  }
  uint32_t mine = 0u;  // keys > T in the low half, real keys == T in the high half
#pragma unroll
  for (int j = 0; j < E; ++j) mine += (q.key[j] > T ? 1u : 0u) + (q.key[j] == T && j < cl ? 0x10000u : 0u);
  uint32_t inc = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  const uint32_t all = __shfl(inc, 63, 64), before = inc - mine;
  const int need = k - (int)(all & 0xffffu);  // ties to take, from the lowest index
  const int total = (int)(all & 0xffffu) + min((int)(all >> 16), need);
  int ties = (int)(before >> 16);
  int slot = (int)(before & 0xffffu) + min(ties, need);
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const bool eq = q.key[j] == T && j < cl;
    const bool sel = q.key[j] > T || (eq && ties < need);
    ties += eq ? 1 : 0;
    const uint32_t u = q.bits(j);
    if (sel) stage[slot] = make_uint2(u, (uint32_t)(lane * E + j));
    slot += sel ? 1 : 0;
    q.key[j] = sel ? 0u : u;  // from here on the new residual
  }
  wave_sync();
  if (lane < k) {
    uint2 t = make_uint2(0u, kEmpty);
    if (lane < total) t = stage[lane];
    s.val[lane] = __uint_as_float(t.x);
    s.off[lane] = (uint16_t)t.y;
  }
  wave_sync();  // the next block's slots go into the same LDS
  if (vec) {
    dev::st_words<E>(err, q.key);
  } else {
#pragma unroll
    for (int j = 0; j < E; ++j)
      if (j < cl) err[j] = __uint_as_float(q.key[j]);
  }
}

// LDS index of element o of the block: plain, or with 4 floats of padding after every lane's run
template <int G, bool PAD>
__device__ __forceinline__ int lds_index(uint32_t o) {
  return PAD ? (int)(o + o / (G / 64) * 4) : (int)o;
}
template <int G, bool PAD>
constexpr int lds_floats() { return PAD ? G + 256 : G; }

// acc (the wave's zeroed LDS block) <- ((d_0 + d_1) + ...) + d_{W-1}, d_r the sparse block b of
// segment r (each `stride` bytes after the one before); true if a version is a skipped (NaN) block
template <int G, bool PAD>
__device__ __forceinline__ bool scatter_sum(const uint8_t* seg, int64_t stride, unsigned cb, unsigned b, int k, int W,
                                            int lane, float* acc) {
  bool nan = false;
  for (int r = 0; r < W; ++r, seg += stride) {
    const Slots s(const_cast<uint8_t*>(seg), cb, b, k);
    if (lane < k) {
      const uint32_t o = s.off[lane];
      const float x = s.val[lane];
      if (o < (uint32_t)G) {
        float* p = acc + lds_index<G, PAD>(o);
        *p = r == 0 ? x : *p + x;  // d_0 itself first: a lone -0 stays -0
      } else {
        nan |= x != x;
      }
    }
    wave_sync();
  }
  return __ballot(nan) != 0ull;
}

template <int N>
__device__ __forceinline__ void zero_lds(float* acc, int lane) {
  const dev::u32x4 z = {0u, 0u, 0u, 0u};
  for (int i = lane * 4; i < N; i += 256) *reinterpret_cast<dev::u32x4*>(acc + i) = z;
  wave_sync();
}

// wave-uniform index of this wave among all waves of the grid
__device__ __forceinline__ unsigned first_block(int waves) {
  return blockIdx.x * waves + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

__device__ __forceinline__ int clampi(int64_t v, int hi) { return v < 0 ? 0 : v > hi ? hi : (int)v; }

// x [n], err [n] -> payload of total = S·cb blocks, of which the first nb are real
template <typename T, int G>
__global__ __launch_bounds__(64 * kTCompressWaves) void topk_compress_kernel(const T* __restrict__ x,
                                                                             float* __restrict__ err,
                                                                             uint8_t* __restrict__ payload, int64_t n,
                                                                             unsigned nb, unsigned cb, unsigned total,
                                                                             int k, int vec) {
  constexpr int E = G / 64;
  __shared__ uint2 stage_all[kTCompressWaves][64];
  const int lane = threadIdx.x & 63;
  uint2* stage = stage_all[threadIdx.x >> 6];
  for (unsigned gb = first_block(kTCompressWaves); gb < total; gb += gridDim.x * kTCompressWaves) {
    const unsigned seg = gb / cb, b = gb - seg * cb;
    const Slots s(payload + (int64_t)seg * cb * k * 6, cb, b, k);
    if (gb >= nb) {
      s.fill(lane, k, 0, 0u);
      continue;
    }
    const int64_t left = n - (int64_t)gb * G;  // >= 1
    const int64_t e0 = (int64_t)gb * G + lane * E;
    const bool whole = vec && left >= G;
    const int cl = clampi(left - lane * E, E);
    Keys<E> q;
    {
      float v[E];
      if (whole) {
        float e[E];
        LaneVec<T, E>::ld(x + e0, v);
        LaneVec<float, E>::ld(err + e0, e);
#pragma unroll
        for (int j = 0; j < E; ++j) v[j] += e[j];
      } else {
#pragma unroll
        for (int j = 0; j < E; ++j) v[j] = j < cl ? dev::Elem<T, float>::ld(x, e0 + j) + err[e0 + j] : 0.f;
      }
      q.set(v);
    }
    select_block<G>(q, cl, k, err + e0, whole, s, stage, lane);
  }
}

// mean (W segments over the same nb blocks) or concat (W = 1, block gb lives in segment gb / cb)
template <typename T, int G>
__global__ __launch_bounds__(64 * lds_waves<G>()) void topk_decode_kernel(const uint8_t* __restrict__ payload,
                                                                          T* __restrict__ out, int64_t n, unsigned nb,
                                                                          unsigned cb, int k, int W, int concat,
                                                                          int vec) {
  constexpr int C = 16 / (int)sizeof(T);  // elements of a 16-byte store
  __shared__ __attribute__((aligned(16))) float lds[lds_waves<G>()][G];
  const int lane = threadIdx.x & 63;
  float* acc = lds[threadIdx.x >> 6];
  const int64_t stride = (int64_t)cb * k * 6;
  const float fw = (float)W;
  for (unsigned gb = first_block(lds_waves<G>()); gb < nb; gb += gridDim.x * lds_waves<G>()) {
    const unsigned seg = concat ? gb / cb : 0u, b = gb - seg * cb;
    zero_lds<G>(acc, lane);
    const bool nan = scatter_sum<G, false>(payload + seg * stride, stride, cb, b, k, W, lane, acc);
    const int64_t base = (int64_t)gb * G;
    const bool whole = vec && base + G <= n;
    for (int i = lane * C; i < G; i += 64 * C) {
      float t[C];
#pragma unroll
      for (int j = 0; j < C; j += 4) {
        const dev::u32x4 a = *reinterpret_cast<const dev::u32x4*>(acc + i + j);
        t[j] = __uint_as_float(a.x); t[j + 1] = __uint_as_float(a.y);
        t[j + 2] = __uint_as_float(a.z); t[j + 3] = __uint_as_float(a.w);
      }
#pragma unroll
      for (int j = 0; j < C; ++j) {
        if (W > 1) t[j] = t[j] / fw;
        if (nan) t[j] = __uint_as_float(kQuietNaN);
      }
      if (whole) {
        LaneVec<T, C>::st(out + base + i, t);
      } else {
#pragma unroll
        for (int j = 0; j < C; ++j)
          if (base + i + j < n) dev::Elem<T, float>::st(out, base + i + j, t[j]);
      }
    }
    wave_sync();  // the next block is zeroed over what was just read
  }
}

// W segments of cb blocks -> one segment: the mean lives in LDS only, takes the server residual
// err [cb·G] and is selected again; the chunk's elements from `numel` on are padding
template <int G>
__global__ __launch_bounds__(64 * lds_waves<G>()) void topk_reduce_reselect_kernel(const uint8_t* __restrict__ in,
                                                                                   float* __restrict__ err,
                                                                                   uint8_t* __restrict__ out,
                                                                                   unsigned cb, int k, int W,
                                                                                   int64_t numel, int vec) {
  constexpr int E = G / 64, N = lds_floats<G, true>();
  __shared__ __attribute__((aligned(16))) float lds[lds_waves<G>()][N];
  __shared__ uint2 stage_all[lds_waves<G>()][64];
  const int lane = threadIdx.x & 63;
  float* acc = lds[threadIdx.x >> 6];
  uint2* stage = stage_all[threadIdx.x >> 6];
  const int64_t stride = (int64_t)cb * k * 6;
  const float fw = (float)W;
  for (unsigned b = first_block(lds_waves<G>()); b < cb; b += gridDim.x * lds_waves<G>()) {
    const Slots s(out, cb, b, k);
    const int64_t left = numel - (int64_t)b * G;
    if (left <= 0) {
      s.fill(lane, k, 0, 0u);
      continue;
    }
    zero_lds<N>(acc, lane);
    if (scatter_sum<G, true>(in, stride, cb, b, k, W, lane, acc)) {  // NaN on a rank: NaN on all, residual kept
      s.fill(lane, k, 0, kQuietNaN);
      continue;
    }
    const int64_t e0 = (int64_t)b * G + lane * E;
    const bool whole = vec && left >= G;
    const int cl = clampi(left - lane * E, E);
    Keys<E> q;
    {
      float v[E];
#pragma unroll
      for (int j = 0; j < E; j += 4) {
        const dev::u32x4 a = *reinterpret_cast<const dev::u32x4*>(acc + lane * (E + 4) + j);
        v[j] = __uint_as_float(a.x); v[j + 1] = __uint_as_float(a.y);
        v[j + 2] = __uint_as_float(a.z); v[j + 3] = __uint_as_float(a.w);
      }
      if (W > 1) {
#pragma unroll
        for (int j = 0; j < E; ++j) v[j] = v[j] / fw;
      }
      if (whole) {
        float e[E];
        LaneVec<float, E>::ld(err + e0, e);
#pragma unroll
        for (int j = 0; j < E; ++j) v[j] += e[j];
      } else {
#pragma unroll
        for (int j = 0; j < E; ++j) v[j] = j < cl ? v[j] + err[e0 + j] : 0.f;
      }
      q.set(v);
    }
    wave_sync();  // all sums are in registers before the LDS block is used again
    select_block<G>(q, cl, k, err + e0, whole, s, stage, lane);
  }
}

// ---- host --------------------------------------------------------------------------------------
int cu_count(int device) {
  int v = 0;
  return hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && v > 0 ? v : 256;
}

dim3 grid_for(int64_t blocks, int waves, int device) {
  const int64_t groups = (blocks + waves - 1) / waves;
  return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(groups, (int64_t)cu_count(device) * kTGroupsPerCU)));
}

void check_format(const char* op, int64_t block, int64_t k, int64_t segments) {
  TORCH_CHECK(block == 1024 || block == 2048 || block == 4096, op, ": block must be 1024, 2048 or 4096, got ", block);
  TORCH_CHECK(k == 8 || k == 16 || k == 32 || k == 64, op, ": k must be 8, 16, 32 or 64, got ", k);
  TORCH_CHECK(segments >= 1 && segments <= 65536, op, ": segments must be in [1, 65536], got ", segments);
}

void check_payload(const char* op, const char* name, const at::Tensor& p, const at::Device& device) {
  TORCH_CHECK(p.is_cuda() && p.device() == device && p.scalar_type() == at::kByte && p.dim() == 1 &&
                  p.is_contiguous(),
              op, ": ", name, " must be a flat contiguous uint8 tensor on ", device);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(p.data_ptr()) % 4 == 0, op, ": ", name, " must be 4-byte aligned");
}

void check_bucket(const char* op, const char* name, const at::Tensor& t) {
  const auto st = t.scalar_type();
  TORCH_CHECK(t.is_cuda() && t.dim() == 1 && t.is_contiguous() &&
                  (st == at::kFloat || st == at::kBFloat16 || st == at::kHalf),
              op, ": ", name, " must be a flat contiguous fp32 / bf16 / fp16 CUDA tensor");
  TORCH_CHECK(t.numel() < (int64_t(1) << 37), op, ": ", name, " has too many elements");  // blocks fit 32 bits
}

void check_err(const char* op, const at::Tensor& err, int64_t numel, const at::Device& device) {
  TORCH_CHECK(err.is_cuda() && err.device() == device && err.scalar_type() == at::kFloat && err.dim() == 1 &&
                  err.is_contiguous(),
              op, ": err must be a flat contiguous fp32 tensor on ", device);
  TORCH_CHECK(err.numel() == numel, op, ": err must hold ", numel, " elements, got ", err.numel());
}

bool aligned16(const at::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }

#define XDDP_TOPK_BLOCK_SWITCH(block, ...)                     \
  switch (block) {                                             \
    case 1024: { constexpr int G = 1024; __VA_ARGS__; break; } \
    case 2048: { constexpr int G = 2048; __VA_ARGS__; break; } \
    default: { constexpr int G = 4096; __VA_ARGS__; break; }   \
  }

template <typename T>
void launch_compress(const at::Tensor& x, at::Tensor& err, at::Tensor& payload, int64_t block, int k, unsigned nb,
                     unsigned cb, unsigned total, hipStream_t stream) {
  const dim3 grid = grid_for(total, kTCompressWaves, x.device().index());
  XDDP_TOPK_BLOCK_SWITCH(block, hipLaunchKernelGGL((topk_compress_kernel<T, G>), grid, dim3(64 * kTCompressWaves), 0,
                                                   stream, reinterpret_cast<const T*>(x.data_ptr()),
                                                   err.data_ptr<float>(), payload.data_ptr<uint8_t>(), x.numel(), nb,
                                                   cb, total, k, aligned16(x) && aligned16(err) ? 1 : 0));
}

template <typename T>
void launch_decode(const at::Tensor& payload, at::Tensor& out, int64_t block, int k, unsigned nb, unsigned cb, int W,
                   int concat, hipStream_t stream) {
  XDDP_TOPK_BLOCK_SWITCH(block, hipLaunchKernelGGL((topk_decode_kernel<T, G>),
                                                   grid_for(nb, lds_waves<G>(), out.device().index()),
                                                   dim3(64 * lds_waves<G>()), 0, stream, payload.data_ptr<uint8_t>(),
                                                   reinterpret_cast<T*>(out.data_ptr()), out.numel(), nb, cb, k, W,
                                                   concat, aligned16(out) ? 1 : 0));
}

}  // namespace

void topk_compress(const at::Tensor& x, at::Tensor err, at::Tensor payload, int64_t block, int64_t k,
                   int64_t segments) {
  check_format("topk_compress", block, k, segments);
  check_bucket("topk_compress", "x", x);
  check_err("topk_compress", err, x.numel(), x.device());
  check_payload("topk_compress", "payload", payload, x.device());
  const int64_t n = x.numel(), nb = (n + block - 1) / block, cb = (nb + segments - 1) / segments;
  const int64_t bpb = 6 * k;
  TORCH_CHECK(payload.numel() == segments * cb * bpb, "topk_compress: payload must hold ", segments * cb * bpb,
              " bytes (", segments, " segments of ", cb, " blocks), got ", payload.numel());
  TORCH_CHECK(segments * cb < (int64_t(1) << 31), "topk_compress: too many blocks");
  if (n == 0) return;
  auto stream = c10::hip::getCurrentHIPStream(x.device().index()).stream();
  const unsigned unb = (unsigned)nb, ucb = (unsigned)cb, total = (unsigned)(segments * cb);
  if (x.scalar_type() == at::kFloat) launch_compress<float>(x, err, payload, block, (int)k, unb, ucb, total, stream);
  else if (x.scalar_type() == at::kBFloat16)
    launch_compress<dev::bf16_t>(x, err, payload, block, (int)k, unb, ucb, total, stream);
  else launch_compress<dev::f16_t>(x, err, payload, block, (int)k, unb, ucb, total, stream);
  XDDP_HIP_CHECK(hipGetLastError());
}

void topk_decode_mean(const at::Tensor& payload, at::Tensor out, int64_t block, int64_t k, int64_t segments,
                      const std::string& mode) {
  check_format("topk_decode_mean", block, k, segments);
  TORCH_CHECK(mode == "mean" || mode == "concat", "topk_decode_mean: mode must be \"mean\" or \"concat\", got \"",
              mode, "\"");
  check_bucket("topk_decode_mean", "out", out);
  check_payload("topk_decode_mean", "payload", payload, out.device());
  const bool concat = mode == "concat";
  const int64_t n = out.numel(), nb = (n + block - 1) / block;
  const int64_t cb = concat ? (nb + segments - 1) / segments : nb;
  const int64_t bpb = 6 * k;
  TORCH_CHECK(payload.numel() == segments * cb * bpb, "topk_decode_mean: payload must hold ", segments * cb * bpb,
              " bytes (", segments, " segments of ", cb, " blocks), got ", payload.numel());
  TORCH_CHECK(segments * cb < (int64_t(1) << 31), "topk_decode_mean: too many blocks");
  if (n == 0) return;
  auto stream = c10::hip::getCurrentHIPStream(out.device().index()).stream();
  const int W = concat ? 1 : (int)segments;
  const unsigned unb = (unsigned)nb, ucb = (unsigned)cb;
  if (out.scalar_type() == at::kFloat) launch_decode<float>(payload, out, block, (int)k, unb, ucb, W, concat, stream);
  else if (out.scalar_type() == at::kBFloat16)
    launch_decode<dev::bf16_t>(payload, out, block, (int)k, unb, ucb, W, concat, stream);
  else launch_decode<dev::f16_t>(payload, out, block, (int)k, unb, ucb, W, concat, stream);
  XDDP_HIP_CHECK(hipGetLastError());
}

void topk_reduce_reselect(const at::Tensor& payload_in, at::Tensor err, at::Tensor payload_out, int64_t block,
                          int64_t k, int64_t segments, int64_t numel) {
  check_format("topk_reduce_reselect", block, k, segments);
  TORCH_CHECK(payload_in.is_cuda(), "topk_reduce_reselect: payload_in must be a CUDA tensor");
  check_payload("topk_reduce_reselect", "payload_in", payload_in, payload_in.device());
  check_payload("topk_reduce_reselect", "payload_out", payload_out, payload_in.device());
  const int64_t seg = payload_out.numel(), bpb = 6 * k;
  TORCH_CHECK(seg % bpb == 0 && payload_in.numel() == segments * seg,
              "topk_reduce_reselect: payload_out must hold whole blocks of ", bpb, " bytes and payload_in ", segments,
              " such segments (", segments * seg, " bytes), got ", seg, " and ", payload_in.numel(), " bytes");
  const int64_t cb = seg / bpb;
  TORCH_CHECK(cb < (int64_t(1) << 31), "topk_reduce_reselect: too many blocks");
  check_err("topk_reduce_reselect", err, cb * block, payload_in.device());
  TORCH_CHECK(numel >= 0 && numel <= cb * block, "topk_reduce_reselect: numel must be in [0, ", cb * block, "], got ",
              numel);
  if (cb == 0) return;
  auto stream = c10::hip::getCurrentHIPStream(payload_in.device().index()).stream();
  XDDP_TOPK_BLOCK_SWITCH(block, hipLaunchKernelGGL((topk_reduce_reselect_kernel<G>),
                                                   grid_for(cb, lds_waves<G>(), payload_in.device().index()),
                                                   dim3(64 * lds_waves<G>()), 0, stream,
                                                   payload_in.data_ptr<uint8_t>(), err.data_ptr<float>(),
                                                   payload_out.data_ptr<uint8_t>(), (unsigned)cb, (int)k,
                                                   (int)segments, numel, aligned16(err) ? 1 : 0));
  XDDP_HIP_CHECK(hipGetLastError());
}

}  // namespace kernels
}  // namespace xddp
