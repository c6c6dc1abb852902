// 16-bit storage formats of the element-wise kernels (the Fmt16 instances of batchnorm.hip and batchnorm2d.hip: bn_fmt.hpp; the *_h max-pool of sparse_aux.hip): widen to fp32 on load,
// round to nearest even ONCE on store.  8 elements travel as one 16-byte access (uint4).
#pragma once
#include "common.hpp"

namespace fv2p {

using u16 = unsigned short;

struct H16 {   // IEEE binary16 (FV2P_DT_F16)
  static __device__ __forceinline__ float widen(u16 v) { return static_cast<float>(__builtin_bit_cast(_Float16, v)); }
  static __device__ __forceinline__ u16 round(float v) { return __builtin_bit_cast(u16, static_cast<_Float16>(v)); }   // v_cvt_f16_f32: nearest even
};
struct B16 {   // bfloat16 (FV2P_DT_BF16)
  static __device__ __forceinline__ float widen(u16 v) { return __uint_as_float(static_cast<unsigned>(v) << 16); }
  static __device__ __forceinline__ u16 round(float v) {   // nearest even on the upper 16 bits; NaN stays a (quiet) NaN
    const unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return static_cast<u16>((u >> 16) | 0x40u);
    return static_cast<u16>((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  }
};

// fp64 -> fp32 rounded to ODD: the inexact result keeps a sticky last bit, so that the nearest-even rounding to 11 or 8 significant
// bits that follows (T::round) sees on which side of a tie the fp64 value lay.  round(to_odd(d)) is the single rounding of d.
__device__ __forceinline__ float to_odd(double d) {
  float f = static_cast<float>(d);
  const double back = static_cast<double>(f);
  if (back != d) {
    unsigned u = __float_as_uint(f);
    if (fabs(back) > fabs(d)) u -= 1u;   // towards zero first (never crosses zero: |f| > |d| > 0)
    f = __uint_as_float(u | 1u);
  }
  return f;
}

// parameter vectors of the BatchNorm kernels: fp32 (pd == 0) or T; a value computed in fp64 is written with ONE rounding
template <class T>
__device__ __forceinline__ float par_load(const void* p, int e, int pd, float dflt) {
  if (!p) return dflt;
  return pd ? T::widen(static_cast<const u16*>(p)[e]) : static_cast<const float*>(p)[e];
}
template <class T>
__device__ __forceinline__ void par_store(void* p, int e, int pd, double v) {
  if (pd) static_cast<u16*>(p)[e] = T::round(to_odd(v));
  else static_cast<float*>(p)[e] = static_cast<float>(v);
}

// V elements of a row: one 16-byte access (V = 8, address 16-byte aligned) or one element (V = 1)
template <class T, int V>
struct Row16;
template <class T>
struct Row16<T, 8> {
  float v[8];
  __device__ __forceinline__ void load(const u16* p) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = T::widen(static_cast<u16>(w[i] & 0xffffu)); v[2 * i + 1] = T::widen(static_cast<u16>(w[i] >> 16)); }
  }
  __device__ __forceinline__ void store(u16* p) const {
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = static_cast<unsigned>(T::round(v[2 * i])) | (static_cast<unsigned>(T::round(v[2 * i + 1])) << 16);
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
};
template <class T>
struct Row16<T, 1> {
  float v[1];
  __device__ __forceinline__ void load(const u16* p) { v[0] = T::widen(*p); }
  __device__ __forceinline__ void store(u16* p) const { *p = T::round(v[0]); }
};

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace fv2p
