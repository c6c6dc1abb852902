// Storage formats of the BatchNorm kernels: batchnorm.hip (rows [N, C]) and batchnorm2d.hip (maps [n, c, hw]) are written once and
// instantiated per format F.  A format supplies the element type, the elements of one 16-byte access (kVec), the unit of V elements
// that one access moves (widened to fp32 on load, rounded to nearest even ONCE on store), `narrow` / `widen` for one element, `stored` (the fp32 value of y as memory
// holds it), how a parameter is read and written (`pd`: fp32, or the tensor's own 16-bit format), and how many rows a thread of the
// row reduction keeps in flight (kRows x 16 bytes per tensor).  The arithmetic is fp32, the sums fp64, in every format.
#pragma once
#include "dt16.hpp"

namespace fv2p {

struct F32 {   // fp32 tensors; the parameters are fp32 (pd is not looked at)
  using elem = float;
  static constexpr int kVec = 4;
  static constexpr int kRows = 8;
  template <int V>
  struct Unit {
    float v[V];
    __device__ __forceinline__ void load(const float* p) {
      if constexpr (V == 4) { const float4 q = *reinterpret_cast<const float4*>(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
      else v[0] = *p;
    }
    __device__ __forceinline__ void store(float* p) const {
      if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
      else *p = v[0];
    }
  };
  static __device__ __forceinline__ float narrow(float v) { return v; }   // fp32 value -> element -> fp32 value
  static __device__ __forceinline__ float widen(float v) { return v; }
  static __device__ __forceinline__ float stored(float y) { return y; }
  static __device__ __forceinline__ float par_load(const void* p, int e, int, float dflt) { return p ? static_cast<const float*>(p)[e] : dflt; }
  static __device__ __forceinline__ void par_store(void* p, int e, int, double v) { static_cast<float*>(p)[e] = static_cast<float>(v); }
};
template <class T>
struct Fmt16 {   // float16 (T = H16) or bfloat16 (B16) tensors; the parameters are fp32 or T (pd)
  using elem = u16;
  static constexpr int kVec = 8;
  static constexpr int kRows = 4;
  template <int V>
  using Unit = Row16<T, V>;
  static __device__ __forceinline__ u16 narrow(float v) { return T::round(v); }
  static __device__ __forceinline__ float widen(u16 v) { return T::widen(v); }
  static __device__ __forceinline__ float stored(float y) { return T::widen(T::round(y)); }
  static __device__ __forceinline__ float par_load(const void* p, int e, int pd, float dflt) { return fv2p::par_load<T>(p, e, pd, dflt); }
  static __device__ __forceinline__ void par_store(void* p, int e, int pd, double v) { fv2p::par_store<T>(p, e, pd, v); }
};

}  // namespace fv2p
