// Lane-private runs of a flat bucket for the gradient-wire kernels (q8_comm.hip, onebit_comm.hip,
// topk_comm.hip):
// one wave owns one block of the format, a lane holds E consecutive elements of it in registers.
#pragma once

#include "kernels/dev_utils.h"

namespace xddp {
namespace dev {

// ---- NW 32-bit words per lane, in the widest accesses their alignment allows ------------------
template <int NW>
__device__ __forceinline__ void ld_words(const void* p, uint32_t (&w)[NW]) {
  if constexpr (NW == 1) {
    w[0] = *reinterpret_cast<const uint32_t*>(p);
  } else if constexpr (NW == 2) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    w[0] = t.x;
    w[1] = t.y;
  } else {
#pragma unroll
    for (int j = 0; j < NW / 4; ++j) {
      const dev::u32x4 t = reinterpret_cast<const dev::u32x4*>(p)[j];
      w[4 * j] = t.x; w[4 * j + 1] = t.y; w[4 * j + 2] = t.z; w[4 * j + 3] = t.w;
    }
  }
}
template <int NW>
__device__ __forceinline__ void st_words(void* p, const uint32_t (&w)[NW]) {
  if constexpr (NW == 1) {
    *reinterpret_cast<uint32_t*>(p) = w[0];
  } else if constexpr (NW == 2) {
    *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
  } else {
#pragma unroll
    for (int j = 0; j < NW / 4; ++j) {
      const dev::u32x4 t = {w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]};
      reinterpret_cast<dev::u32x4*>(p)[j] = t;
    }
  }
}

// a lane's E elements of the bucket as fp32 (p is aligned to min(16, E·sizeof(T)) bytes)
template <typename T, int E>
struct LaneVec {
  static constexpr int NW = E * (int)sizeof(T) / 4;
  static __device__ __forceinline__ void ld(const T* p, float (&v)[E]) {
    uint32_t w[NW];
    ld_words<NW>(p, w);
    if constexpr (sizeof(T) == 4) {
#pragma unroll
      for (int k = 0; k < E; ++k) v[k] = __uint_as_float(w[k]);
    } else {
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        if constexpr (__is_same(T, dev::bf16_t)) {
          v[2 * j] = __uint_as_float(w[j] << 16);
          v[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
        } else {
          v[2 * j] = dev::f16_to_f32((uint16_t)(w[j] & 0xffffu));
          v[2 * j + 1] = dev::f16_to_f32((uint16_t)(w[j] >> 16));
        }
      }
    }
  }
  static __device__ __forceinline__ void st(T* p, const float (&v)[E]) {
    uint32_t w[NW];
    if constexpr (sizeof(T) == 4) {
#pragma unroll
      for (int k = 0; k < E; ++k) w[k] = __float_as_uint(v[k]);
    } else {
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        if constexpr (__is_same(T, dev::bf16_t)) w[j] = dev::pack_bf16x2(v[2 * j], v[2 * j + 1]);
        else w[j] = dev::pack_f16x2(v[2 * j], v[2 * j + 1]);
      }
    }
    st_words<NW>(p, w);
  }
};

}  // namespace dev
}  // namespace xddp
