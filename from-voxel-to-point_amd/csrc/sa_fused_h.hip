// Fused grid set-abstraction on 16-bit rows (float16 / bfloat16) for gfx950: fv2p_sa_grid_fwd_h / fv2p_sa_grid_bwd_h (include/fv2p_ops.h),
// the siblings of sa_fused.hip's fp32 entry points, which this file does not touch.
//        out[r, i, :] = max_s relu(W2 relu(P[r, idx[r, i, s], :] - Q[r, i, :]))         P (R, N, 64), Q / out (R, M, 64), S in {16, 32}
// P, Q, out and every gradient are stored in ONE 16-bit format T; W2 (64, 64) is T (wd != 0) or fp32 (wd == 0: the master weight an
// autocast caller has).  fp32 weights are rounded to T on their way into LDS - the bits of W2.to(T); no 16-bit copy exists in memory -
// and no fp32 image of P, Q, out or a gradient is made anywhere.
//
// Arithmetic of the forward (the contract of tests/test_sa_half_gpu.py):
//   h1      = RNE_T(max(float(P) - float(Q), 0))    fp32 subtraction of the widened values, rounded once: the MFMA operand
//   a[s][o] = sum_c W2r[o][c] h1[s][c]              fp32 accumulators of v_mfma_f32_16x16x32_{f16,bf16}; a product of two T values is exact
//   out     = RNE_T(max(0, max_s a[s][o]))          the maximum over the fp32 accumulators, rounded once at the store
//   arg     = the first sample in sample order whose fp32 accumulator equals the maximum; 255 where the maximum is 0
//             (fv2p_sa_grid_fwd's definition: ties between repeated indices go to the earliest slot)
// An index outside [0, N) reads as a row of zeros (h1 = relu(-Q)); it is never dereferenced, and backward drops its dh1 entry.
//
// Layout.  As in the fp32 kernel the product is formed transposed, h2^T = W2 h1^T: the 16 sample rows of a tile are the 16 lanes of a
// DPP row, and lane (row = l & 15, g = l >> 4) receives the channels 16 b + 4 g + e (b, e = 0..3) of its sample row in the accumulators.
// The 16x16x32 MFMA wants 8 contraction indices per lane and K step; the order of K inside an MFMA is free as long as A and B agree, so
// K index (step ks, g, j) stands for channel 32 ks + 16 (j >> 2) + 4 g + (j & 3): a lane's B operand is then the SAME 16 channels
// 16 b + 4 g + e it receives results for - four 8-byte loads of a 128-byte row, four lanes covering 32 contiguous bytes - and results
// chain into the next product (backward: dh1^T = W2^T dh2^T) and meet the mask [h1 > 0] without a shuffle.  The W2 (forward) and W2^T
// (backward) fragments are staged in LDS in that permutation, 8 KB, one 16-byte read per lane, block and K step.  8 MFMAs per tile of
// 16 samples instead of the fp32 kernel's 64.
//
// Backward recomputes h1 exactly as forward, routes the 16-bit values of grad_out to the sample arg names (dh2, exact), and gives
//   dh1         = (W2r^T dh2) [h1 > 0]              16-bit MFMA, fp32 accumulators
//   grad_centre = -sum_s dh1                        fp32 sum over the tiles, then over the DPP row in a fixed order; one rounding
//   grad_point  : every (centre, sample) row of dh1 is rounded to T and STAGED IN 16 BITS in the workspace (one more rounding per addend:
//                 u_s = u in the tests' bound), then summed per point in fp32 in a fixed order and rounded once.  Up to 8192 samples per
//                 RoI (the head has 3456 / 6912) a workgroup per RoI sorts the RoI's (point, sample) keys in LDS and adds each point's rows
//                 in ascending sample order (sa_grid_points_h_k); beyond that scatter_add_h does it in the association of
//                 fv2p_scatter_add.  No atomics of any kind, no sums in LDS, no dP tile, hence no limit on N; there is no atomic form, and
//                 the deterministic switch changes nothing.
//   grad_w2[o][c] = sum_{r,i,s} dh2[o] h1[c]        sample rows are the K dimension: both tiles go through LDS transposed ([channel][sample
//                 row], wave-private), one K = 32 step per centre (an S = 16 centre fills half of it, the other half stays zero); fp32 partial
//                 tile per workgroup (the four waves folded as (w0 + w2) + (w1 + w3)), the partials folded in a fixed order by
//                 sa_dw_fold_h_k (sa_grid_dw_reduce_k's scheme) and written in W2's dtype: one rounding for a 16-bit weight, none for fp32.
// Every result has the same bits from run to run and on any stream.
#include "common.hpp"
#include "dt16.hpp"

namespace fv2p {
namespace {

using f32x4 = float __attribute__((ext_vector_type(4)));
using f16x8 = _Float16 __attribute__((ext_vector_type(8)));
using bf16x8 = __bf16 __attribute__((ext_vector_type(8)));

struct MH : H16 {
  static __device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};
struct MB : B16 {
  // gfx950 converts in hardware (v_cvt_pk_bf16_f32: nearest even, NaN stays a quiet NaN): the bits of B16::round
  static __device__ __forceinline__ u16 round(float v) { return __builtin_bit_cast(u16, static_cast<__bf16>(v)); }
  static __device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};

constexpr int kC = 64;             // channels of both layers
constexpr int kFwdCentres = 16;    // centres per workgroup, forward
constexpr int kBwdCentres = 64;    // centres per workgroup, backward (one fp32 dW2 partial tile each)
constexpr int kLd = 40;            // row stride of the transposed tiles in elements: 32 sample rows + 8 (80-byte rows, 16-byte aligned)

// Reductions over the 16 lanes of a DPP row (the 16 sample rows of a tile), step-major: quad_perm xor-1, xor-2, row_half_mirror,
// row_mirror.  Every lane of the row ends with the row's result, and the association is the same in every lane and every launch.
template <int CTRL>
__device__ __forceinline__ float dpp_of(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ void row16_max_step(float (&v)[16]) {
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = fmaxf(v[k], dpp_of<CTRL>(v[k]));
}
template <int CTRL>
__device__ __forceinline__ void row16_sum_step(float (&v)[16]) {
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = v[k] + dpp_of<CTRL>(v[k]);
}
__device__ __forceinline__ void row16_max_n(float (&v)[16]) {
  row16_max_step<0xB1>(v); row16_max_step<0x4E>(v); row16_max_step<0x141>(v); row16_max_step<0x140>(v);
}
__device__ __forceinline__ void row16_sum_n(float (&v)[16]) {
  row16_sum_step<0xB1>(v); row16_sum_step<0x4E>(v); row16_sum_step<0x141>(v); row16_sum_step<0x140>(v);
}

template <class T, bool W32>
__device__ __forceinline__ unsigned w_at(const void* __restrict__ w, int o, int c) {
  if constexpr (W32) return T::round(static_cast<const float*>(w)[o * kC + c]);
  else return static_cast<const u16*>(w)[o * kC + c];
}
// LDS image of W2 (TR = false) or W2^T (TR = true) as the A operand: frag[b][ks][lane] (8 elements) = A[16 b + lane % 16][k], k the
// permuted channel 32 ks + 16 (j >> 2) + 4 (lane / 16) + (j & 3), j = 0..7
template <class T, bool W32, bool TR>
__device__ __forceinline__ void stage_w(const void* __restrict__ w, u16* __restrict__ lds) {
  for (int e = threadIdx.x; e < 8 * 64; e += 256) {
    const int lane = e & 63, ks = (e >> 6) & 1, b = e >> 7;
    const int rw = 16 * b + (lane & 15), g = lane >> 4;
    unsigned wv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k0 = 32 * ks + 16 * (i >> 1) + 4 * g + 2 * (i & 1);
      const unsigned lo = TR ? w_at<T, W32>(w, k0, rw) : w_at<T, W32>(w, rw, k0);
      const unsigned hi = TR ? w_at<T, W32>(w, k0 + 1, rw) : w_at<T, W32>(w, rw, k0 + 1);
      wv[i] = lo | (hi << 16);
    }
    *reinterpret_cast<uint4*>(lds + e * 8) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
  }
}

__device__ __forceinline__ uint2 load8(const u16* p) { return *reinterpret_cast<const uint2*>(p); }
template <class T>
__device__ __forceinline__ void widen4(uint2 v, float (&f)[4]) {
  f[0] = T::widen(static_cast<u16>(v.x & 0xffffu)); f[1] = T::widen(static_cast<u16>(v.x >> 16));
  f[2] = T::widen(static_cast<u16>(v.y & 0xffffu)); f[3] = T::widen(static_cast<u16>(v.y >> 16));
}
template <class T>
__device__ __forceinline__ uint2 round4(float a, float b, float c, float d) {
  return make_uint2(static_cast<unsigned>(T::round(a)) | (static_cast<unsigned>(T::round(b)) << 16),
                    static_cast<unsigned>(T::round(c)) | (static_cast<unsigned>(T::round(d)) << 16));
}
// h1 = RNE_T(max(p - q, 0)) for four channels
template <class T>
__device__ __forceinline__ uint2 relu_sub(uint2 p, const float (&q)[4]) {
  float f[4];
  widen4<T>(p, f);
  return round4<T>(fmaxf(f[0] - q[0], 0.f), fmaxf(f[1] - q[1], 0.f), fmaxf(f[2] - q[2], 0.f), fmaxf(f[3] - q[3], 0.f));
}
__device__ __forceinline__ unsigned elem16(uint2 v, int e) { return ((e < 2 ? v.x : v.y) >> (16 * (e & 1))) & 0xffffu; }

// acc[b] += A-fragments(lds)[b][ks] * x   (x[b] = this lane's channels 16 b + 4 g .. + 3 of its sample row)
template <class T>
__device__ __forceinline__ void mma64(const u16* __restrict__ frag, int lane, const uint2 (&x)[4], f32x4 (&acc)[4]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const uint4 bop = make_uint4(x[2 * ks].x, x[2 * ks].y, x[2 * ks + 1].x, x[2 * ks + 1].y);
    uint4 a[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) a[b] = *reinterpret_cast<const uint4*>(frag + ((b * 2 + ks) * 64 + lane) * 8);
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = T::mfma(a[b], bop, acc[b]);
  }
}

// ------------------------------------------------------------------ forward ---------------------------------------------------
// grid (ceil(M / 16), R), block 256: wave w handles centres 16 * blockIdx.x + w, w + 4, ...
template <class T, int TILES, bool W32>
__global__ __launch_bounds__(256) void sa_grid_fwd_h_k(int n, int m, const u16* __restrict__ P, const u16* __restrict__ Q, const int* __restrict__ idx,
                                                       const void* __restrict__ W2, u16* __restrict__ out, unsigned char* __restrict__ arg) {
  __shared__ __attribute__((aligned(16))) u16 wfrag[8 * 64 * 8];
  constexpr int s = 16 * TILES;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, g = lane >> 4;
  const int r = blockIdx.y;
  stage_w<T, W32, false>(W2, wfrag);
  __syncthreads();
  const u16* Pr = P + static_cast<long long>(r) * n * kC;
  for (int ci = wave; ci < kFwdCentres; ci += 4) {
    const int i = blockIdx.x * kFwdCentres + ci;
    if (i >= m) break;
    const long long ctr = static_cast<long long>(r) * m + i;
    int src[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t) src[t] = idx[ctr * s + 16 * t + row];
    uint2 qraw[4], praw[TILES][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) qraw[b] = load8(Q + ctr * kC + 16 * b + 4 * g);
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      const bool ok = static_cast<unsigned>(src[t]) < static_cast<unsigned>(n);   // outside [0, n): a row of zeros, never dereferenced
      const u16* p = Pr + static_cast<long long>(ok ? src[t] : 0) * kC + 4 * g;
#pragma unroll
      for (int b = 0; b < 4; ++b) praw[t][b] = ok ? load8(p + 16 * b) : make_uint2(0u, 0u);
    }
    float qf[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) widen4<T>(qraw[b], qf[b]);
    float best[16];
    uint32_t late = 0;   // bit 4 b + e: this lane's best value of that channel came from the second tile
#pragma unroll
    for (int k = 0; k < 16; ++k) best[k] = 0.f;   // relu output: the maximum is >= 0
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      uint2 x[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) x[b] = relu_sub<T>(praw[t][b], qf[b]);
      f32x4 acc[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
      mma64<T>(wfrag, lane, x, acc);
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (t != 0 && acc[b][e] > best[4 * b + e]) late |= 1u << (4 * b + e);   // strict: the earlier sample keeps a tie
          best[4 * b + e] = fmaxf(best[4 * b + e], acc[b][e]);
        }
    }
    // lane (row, g) holds channels 16 b + 4 g + e of sample row `row`: maximum over the 16 lanes of the DPP row
    float flat[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) flat[k] = best[k];
    row16_max_n(flat);
    if (row == 0) {
      u16* o = out + ctr * kC + 4 * g;
#pragma unroll
      for (int b = 0; b < 4; ++b) *reinterpret_cast<uint2*>(o + 16 * b) = round4<T>(flat[4 * b], flat[4 * b + 1], flat[4 * b + 2], flat[4 * b + 3]);
    }
    if (arg) {
      // first sample (in sample order) that attains the maximum: lanes holding it offer -(their sample number), the row maximum of
      // that is the smallest number; a lane's own first is its first tile unless the second was strictly larger
      float cand[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const bool holds = best[k] == flat[k] && flat[k] > 0.f;
        cand[k] = holds ? -static_cast<float>(((late >> k) & 1u) * 16u + static_cast<uint32_t>(row)) : -255.f;
      }
      row16_max_n(cand);
      if (row == 0) {
        unsigned char* a = arg + ctr * kC + 4 * g;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const uint32_t packed = static_cast<uint32_t>(-cand[4 * b]) | (static_cast<uint32_t>(-cand[4 * b + 1]) << 8) |
                                  (static_cast<uint32_t>(-cand[4 * b + 2]) << 16) | (static_cast<uint32_t>(-cand[4 * b + 3]) << 24);
          *reinterpret_cast<uint32_t*>(a + 16 * b) = packed;
        }
      }
    }
  }
}

// ------------------------------------------------------------------ backward --------------------------------------------------
// grid (ceil(M / 64), R), block 256: wave w takes centres 64 * blockIdx.x + w, w + 4, ...  LDS: the W2^T fragments (8 KB) and per wave
// two transposed tiles [64 channels][kLd] (dh2, h1: 10 KB), 48 KB; the fold of the waves' dW2 accumulators reuses it.
constexpr int kBwdLds = 8 * 64 * 8 * 2 + 4 * 2 * kC * kLd * 2;

template <class T, int TILES, bool W32>
__global__ __launch_bounds__(256) void sa_grid_bwd_h_k(int n, int m, const u16* __restrict__ P, const u16* __restrict__ Q, const int* __restrict__ idx,
                                                       const void* __restrict__ W2, const unsigned char* __restrict__ arg,
                                                       const u16* __restrict__ dout, u16* __restrict__ dQ, float* __restrict__ dW2_partial,
                                                       u16* __restrict__ dh1_rows) {
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[kBwdLds];
  constexpr int s = 16 * TILES;
  u16* wtfrag = reinterpret_cast<u16*>(lds_raw);
  u16* tiles = wtfrag + 8 * 64 * 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, g = lane >> 4;
  const int r = blockIdx.y;
  stage_w<T, W32, true>(W2, wtfrag);
  for (int e = threadIdx.x; e < 4 * 2 * kC * kLd / 2; e += 256) reinterpret_cast<uint32_t*>(tiles)[e] = 0u;   // S = 16: sample rows 16 .. 31 stay zero
  __syncthreads();
  u16* t_dh2 = tiles + wave * 2 * kC * kLd;
  u16* t_h1 = t_dh2 + kC * kLd;
  const u16* Pr = P + static_cast<long long>(r) * n * kC;
  f32x4 dw[4][4];   // dW2[16 bo + 4 g + e][16 bc + row], summed over every sample row this wave sees
#pragma unroll
  for (int bo = 0; bo < 4; ++bo)
#pragma unroll
    for (int bc = 0; bc < 4; ++bc) dw[bo][bc] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int c0 = blockIdx.x * kBwdCentres, c1 = c0 + kBwdCentres < m ? c0 + kBwdCentres : m;
  for (int i = c0 + wave; i < c1; i += 4) {
    const long long ctr = static_cast<long long>(r) * m + i;
    int src[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t) src[t] = idx[ctr * s + 16 * t + row];
    uint2 qraw[4], graw[4], praw[TILES][4];
    uint32_t who[4];   // byte e of who[b]: the sample that attained the maximum of channel 16 b + 4 g + e (255: none)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      qraw[b] = load8(Q + ctr * kC + 16 * b + 4 * g);
      graw[b] = load8(dout + ctr * kC + 16 * b + 4 * g);
      who[b] = *reinterpret_cast<const uint32_t*>(arg + ctr * kC + 16 * b + 4 * g);
    }
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      const bool ok = static_cast<unsigned>(src[t]) < static_cast<unsigned>(n);
      const u16* p = Pr + static_cast<long long>(ok ? src[t] : 0) * kC + 4 * g;
#pragma unroll
      for (int b = 0; b < 4; ++b) praw[t][b] = ok ? load8(p + 16 * b) : make_uint2(0u, 0u);
    }
    float qf[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) widen4<T>(qraw[b], qf[b]);
    float dq[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) dq[k] = 0.f;
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      uint2 x[4], dh2[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        x[b] = relu_sub<T>(praw[t][b], qf[b]);
        unsigned d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = ((who[b] >> (8 * e)) & 0xffu) == static_cast<uint32_t>(16 * t + row) ? elem16(graw[b], e) : 0u;
        dh2[b] = make_uint2(d[0] | (d[1] << 16), d[2] | (d[3] << 16));
      }
      f32x4 d1[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) d1[b] = f32x4{0.f, 0.f, 0.f, 0.f};
      mma64<T>(wtfrag, lane, dh2, d1);   // dh1^T = W2^T dh2^T: channels 16 b + 4 g + e of this lane's sample row
      u16* ro = dh1_rows + ((ctr * s + 16 * t + row) * kC + 4 * g);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = (elem16(x[b], e) & 0x7fffu) != 0u ? d1[b][e] : 0.f;   // [h1 > 0] on the rounded h1 (never negative; -0 counts as 0)
          dq[4 * b + e] += v[e];
        }
        *reinterpret_cast<uint2*>(ro + 16 * b) = round4<T>(v[0], v[1], v[2], v[3]);
        // dW2 += dh2^T h1 needs the sample rows as the K dimension: both tiles transposed through LDS, [channel][sample row]
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          t_h1[(16 * b + 4 * g + e) * kLd + 16 * t + row] = static_cast<u16>(elem16(x[b], e));
          t_dh2[(16 * b + 4 * g + e) * kLd + 16 * t + row] = static_cast<u16>(elem16(dh2[b], e));
        }
      }
    }
    __builtin_amdgcn_wave_barrier();   // the tiles are private to the wave; LDS serves a wave's accesses in order
    {
      uint4 a[4], bf[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a[q] = *reinterpret_cast<const uint4*>(t_dh2 + (16 * q + row) * kLd + 8 * g);    // A[m = o % 16][k = sample row 8 g + j]
        bf[q] = *reinterpret_cast<const uint4*>(t_h1 + (16 * q + row) * kLd + 8 * g);    // B[k = sample row 8 g + j][n = c % 16]
      }
#pragma unroll
      for (int bo = 0; bo < 4; ++bo)
#pragma unroll
        for (int bc = 0; bc < 4; ++bc) dw[bo][bc] = T::mfma(a[bo], bf[bc], dw[bo][bc]);
    }
    __builtin_amdgcn_wave_barrier();
    // dQ[i][c] = - sum over the centre's samples of dh1 (the 16 lanes of the DPP row)
    row16_sum_n(dq);
    if (row == 0) {
      u16* dqo = dQ + ctr * kC + 4 * g;
#pragma unroll
      for (int b = 0; b < 4; ++b) *reinterpret_cast<uint2*>(dqo + 16 * b) = round4<T>(-dq[4 * b], -dq[4 * b + 1], -dq[4 * b + 2], -dq[4 * b + 3]);
    }
  }
  // dW2 partial of this workgroup: (w0 + w2) + (w1 + w3) through LDS (fragments and tiles are free now)
  __syncthreads();
  float* buf = reinterpret_cast<float*>(lds_raw);   // two waves' accumulators: 32 KB
  auto put = [&](int slot) {
#pragma unroll
    for (int bo = 0; bo < 4; ++bo)
#pragma unroll
      for (int bc = 0; bc < 4; ++bc) *reinterpret_cast<f32x4*>(buf + (((slot * 4 + bo) * 4 + bc) * 64 + lane) * 4) = dw[bo][bc];
  };
  auto add = [&](int slot) {
#pragma unroll
    for (int bo = 0; bo < 4; ++bo)
#pragma unroll
      for (int bc = 0; bc < 4; ++bc) {
        const f32x4 o = *reinterpret_cast<const f32x4*>(buf + (((slot * 4 + bo) * 4 + bc) * 64 + lane) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) dw[bo][bc][e] = dw[bo][bc][e] + o[e];
      }
  };
  if (wave >= 2) put(wave - 2);
  __syncthreads();
  if (wave < 2) add(wave);
  __syncthreads();
  if (wave == 1) put(0);
  __syncthreads();
  if (wave == 0) {
    add(0);
    float* dwo = dW2_partial + (static_cast<long long>(r) * gridDim.x + blockIdx.x) * (kC * kC);
#pragma unroll
    for (int bo = 0; bo < 4; ++bo)
#pragma unroll
      for (int bc = 0; bc < 4; ++bc)
#pragma unroll
        for (int e = 0; e < 4; ++e) dwo[(16 * bo + 4 * g + e) * kC + 16 * bc + row] = dw[bo][bc][e];
  }
}

// dW2 = the column sums of the partial tiles [parts][64 * 64] in sa_grid_dw_reduce_k's fixed association: a workgroup owns 16 columns,
// its 256 threads are 16 row groups x 16 columns, a thread adds the rows rg, rg + 16, ... in ascending order and the 16 group sums are
// added in group order.  Written in W2's dtype: fp32 as it is (wd == 0) or rounded once.
template <class T>
__global__ __launch_bounds__(256) void sa_dw_fold_h_k(int parts, const float* __restrict__ partial, void* __restrict__ dW2, int wd) {
  __shared__ float part[16][17];
  const int col = blockIdx.x * 16 + (threadIdx.x & 15), rg = threadIdx.x >> 4;
  float s = 0.f;
  for (int p = rg; p < parts; p += 16) s += partial[static_cast<long long>(p) * (kC * kC) + col];
  part[rg][threadIdx.x & 15] = s;
  __syncthreads();
  if (threadIdx.x < 16) {
    float v = part[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < 16; ++q) v += part[q][threadIdx.x];
    if (wd) static_cast<u16*>(dW2)[blockIdx.x * 16 + threadIdx.x] = T::round(v);
    else static_cast<float*>(dW2)[blockIdx.x * 16 + threadIdx.x] = v;
  }
}

// grad_point of one RoI inside one workgroup, for M * S <= 8192 samples per RoI and N <= 2^18: grid (R), block 512.  The RoI's samples
// become keys (point << 13 | sample number) - unique, so the bitonic sort in LDS has ONE result - and a point's samples are then one run
// in ascending sample number.  Eight lanes (16 bytes of the 128-byte row each) own a point: they add its staged dh1 rows in that order
// in fp32, starting from zero, round once and write the row (zeros for a point no sample names: grad_point needs no fill).  Nothing is
// added in LDS or with atomics; the association is a function of idx alone.
constexpr int kPtBits = 13, kPtMax = 1 << kPtBits, kPtMaxN = 1 << 18;
template <class T>
__global__ __launch_bounds__(512) void sa_grid_points_h_k(int n, int per_roi, int len, const int* __restrict__ idx, const u16* __restrict__ rows,
                                                          u16* __restrict__ dP) {
  __shared__ uint32_t keys[kPtMax];
  const int r = blockIdx.x;
  const int* id = idx + static_cast<long long>(r) * per_roi;
  for (int e = threadIdx.x; e < len; e += 512) {   // len: the power of two at or above per_roi; the padding and dropped samples sort last
    uint32_t k = 0xffffffffu;
    if (e < per_roi) {
      const int p = id[e];
      if (static_cast<unsigned>(p) < static_cast<unsigned>(n)) k = (static_cast<uint32_t>(p) << kPtBits) | static_cast<uint32_t>(e);
    }
    keys[e] = k;
  }
  __syncthreads();
  for (int k = 2; k <= len; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (len >> 1); t += 512) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint32_t a = keys[i], b = keys[l];
        if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[l] = a; }
      }
      __syncthreads();
    }
  auto lower_bound = [&](uint32_t target, int lo) {
    int hi = len;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] < target) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  const int grp = threadIdx.x >> 3, l8 = threadIdx.x & 7;
  const u16* rr = rows + static_cast<long long>(r) * per_roi * kC + 8 * l8;
  for (int p = grp; p < n; p += 64) {
    const int lo = lower_bound(static_cast<uint32_t>(p) << kPtBits, 0), hi = lower_bound(static_cast<uint32_t>(p + 1) << kPtBits, lo);
    Row16<T, 8> acc;
#pragma unroll
    for (int q = 0; q < 8; ++q) acc.v[q] = 0.f;
    int k = lo;
    for (; k + 4 <= hi; k += 4) {   // four loads in flight, added in sample order
      Row16<T, 8> v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u].load(rr + static_cast<long long>(keys[k + u] & (kPtMax - 1)) * kC);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int q = 0; q < 8; ++q) acc.v[q] = acc.v[q] + v[u].v[q];
    }
    for (; k < hi; ++k) {
      Row16<T, 8> v;
      v.load(rr + static_cast<long long>(keys[k] & (kPtMax - 1)) * kC);
#pragma unroll
      for (int q = 0; q < 8; ++q) acc.v[q] = acc.v[q] + v.v[q];
    }
    acc.store(dP + (static_cast<long long>(r) * n + p) * kC + 8 * l8);
  }
}

// entry e = (r * m + i) * s + sample of the dh1 rows -> row r * n + idx[e] of grad_point (dropped outside [0, n))
__global__ void sa_grid_entries_h_k(int64_t entries, int n, int64_t per_roi, const int* __restrict__ idx, int* __restrict__ dst) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= entries) return;
  const int i = idx[e];
  dst[e] = i >= 0 && i < n ? static_cast<int>((e / per_roi) * n + i) : -1;
}

bool shapes_ok(int rois, int n, int m, int s, int c) {
  return rois >= 1 && rois <= 65535 && n >= 1 && m >= 1 && c == kC && (s == 16 || s == 32);
}
int chunks_of(int m) { return static_cast<int>(ceil_div(m > 0 ? m : 1, kBwdCentres)); }

template <class T, int TILES, bool W32>
void launch_fwd(const void* P, const void* Q, const int* idx, const void* w2, int rois, int n, int m, void* out, unsigned char* arg, hipStream_t st) {
  hipLaunchKernelGGL((sa_grid_fwd_h_k<T, TILES, W32>), dim3(static_cast<unsigned>(ceil_div(m, kFwdCentres)), rois), dim3(256), 0, st, n, m,
                     static_cast<const u16*>(P), static_cast<const u16*>(Q), idx, w2, static_cast<u16*>(out), arg);
}
template <class T, int TILES, bool W32>
void launch_bwd(const void* P, const void* Q, const int* idx, const void* w2, const unsigned char* arg, const void* go, int rois, int n, int m,
                void* dQ, float* partial, u16* rows, hipStream_t st) {
  hipLaunchKernelGGL((sa_grid_bwd_h_k<T, TILES, W32>), dim3(static_cast<unsigned>(chunks_of(m)), rois), dim3(256), 0, st, n, m,
                     static_cast<const u16*>(P), static_cast<const u16*>(Q), idx, w2, arg, static_cast<const u16*>(go), static_cast<u16*>(dQ), partial, rows);
}

}  // namespace
}  // namespace fv2p
using namespace fv2p;

#define FV2P_SA_H_DISPATCH(fn, ...)                                                                     \
  do {                                                                                                  \
    if (dtype == FV2P_DT_F16) {                                                                         \
      if (s == 16) { if (wd) fn<MH, 1, false>(__VA_ARGS__); else fn<MH, 1, true>(__VA_ARGS__); }        \
      else { if (wd) fn<MH, 2, false>(__VA_ARGS__); else fn<MH, 2, true>(__VA_ARGS__); }                \
    } else {                                                                                            \
      if (s == 16) { if (wd) fn<MB, 1, false>(__VA_ARGS__); else fn<MB, 1, true>(__VA_ARGS__); }        \
      else { if (wd) fn<MB, 2, false>(__VA_ARGS__); else fn<MB, 2, true>(__VA_ARGS__); }                \
    }                                                                                                   \
  } while (0)

extern "C" int fv2p_sa_grid_supported_h(int n, int m, int s, int c) {
  return (c == kC && (s == 16 || s == 32) && n >= 1 && m >= 1) ? 1 : 0;   // no dP tile in LDS: no limit on n
}

extern "C" int fv2p_sa_grid_fwd_h(const void* per_point, const void* per_centre, const int* idx, const void* w2, int wd, int rois, int n, int m,
                                  int s, int c, void* out, unsigned char* arg, int dtype, fv2p_stream_t stream) {
  FV2P_DT16_OK("sa_grid_fwd_h", dtype);
  FV2P_REQUIRE(wd == 0 || wd == dtype, FV2P_EINVAL, "sa_grid_fwd_h: w2 is fp32 (wd 0) or has the rows' dtype, got wd %d beside dtype %d", wd, dtype);
  FV2P_REQUIRE(shapes_ok(rois, n, m, s, c), FV2P_EINVAL, "sa_grid_fwd_h: needs 64 channels and 16 or 32 samples per centre");
  FV2P_REQUIRE(per_point && per_centre && idx && w2 && out, FV2P_EINVAL, "sa_grid_fwd_h: null pointer");
  FV2P_REQUIRE(aligned16(per_point) && aligned16(per_centre) && aligned16(out) && aligned16(w2) && aligned16(arg), FV2P_EINVAL,
               "sa_grid_fwd_h: rows must be 16-byte aligned");
  FV2P_SA_H_DISPATCH(launch_fwd, per_point, per_centre, idx, w2, rois, n, m, out, arg, static_cast<hipStream_t>(stream));
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t fv2p_sa_grid_bwd_h_ws_bytes(int rois, int m, int s) {
  const size_t r = static_cast<size_t>(rois > 0 ? rois : 1);
  const int64_t entries = static_cast<int64_t>(r) * (m > 0 ? m : 1) * (s > 0 ? s : 1);
  Sizer sz;
  sz.take<float>(r * chunks_of(m) * kC * kC);
  sz.take<int>(static_cast<size_t>(entries));
  sz.take<u16>(static_cast<size_t>(entries) * kC);
  sz.take<char>(fv2p_scatter_add_ws_bytes(entries, kC));
  return sz.bytes();
}

extern "C" int fv2p_sa_grid_bwd_h(const void* per_point, const void* per_centre, const int* idx, const void* w2, int wd, const unsigned char* arg,
                                  const void* grad_out, int rois, int n, int m, int s, int c, void* grad_point, void* grad_centre, void* grad_w2,
                                  int dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FV2P_DT16_OK("sa_grid_bwd_h", dtype);
  FV2P_REQUIRE(wd == 0 || wd == dtype, FV2P_EINVAL, "sa_grid_bwd_h: w2 is fp32 (wd 0) or has the rows' dtype, got wd %d beside dtype %d", wd, dtype);
  FV2P_REQUIRE(shapes_ok(rois, n, m, s, c), FV2P_EINVAL, "sa_grid_bwd_h: needs 64 channels and 16 or 32 samples per centre");
  FV2P_REQUIRE(per_point && per_centre && idx && w2 && arg && grad_out && grad_point && grad_centre && grad_w2, FV2P_EINVAL, "sa_grid_bwd_h: null pointer");
  FV2P_REQUIRE(aligned16(per_point) && aligned16(per_centre) && aligned16(grad_out) && aligned16(w2) && aligned16(arg) && aligned16(grad_centre) &&
                   aligned16(grad_point) && aligned16(grad_w2), FV2P_EINVAL, "sa_grid_bwd_h: rows must be 16-byte aligned");
  const int64_t entries = static_cast<int64_t>(rois) * m * s;
  FV2P_REQUIRE(entries < (1ll << 31) && static_cast<int64_t>(rois) * n < (1ll << 31) - 1, FV2P_ELIMIT, "sa_grid_bwd_h: too many samples");
  FV2P_REQUIRE(ws && ws_bytes >= fv2p_sa_grid_bwd_h_ws_bytes(rois, m, s), FV2P_EWORKSPACE, "sa_grid_bwd_h: workspace too small");
  Carver cv(ws, ws_bytes);
  const int parts = rois * chunks_of(m);
  float* partial = cv.take<float>(static_cast<size_t>(parts) * kC * kC);
  int* dst = cv.take<int>(static_cast<size_t>(entries));
  u16* rows = cv.take<u16>(static_cast<size_t>(entries) * kC);
  const size_t sb = fv2p_scatter_add_ws_bytes(entries, kC);
  void* sws = cv.take<char>(sb);
  FV2P_SA_H_DISPATCH(launch_bwd, per_point, per_centre, idx, w2, arg, grad_out, rois, n, m, grad_centre, partial, rows, stream);
  if (dtype == FV2P_DT_F16) hipLaunchKernelGGL(sa_dw_fold_h_k<MH>, dim3(kC * kC / 16), dim3(256), 0, stream, parts, partial, grad_w2, wd);
  else hipLaunchKernelGGL(sa_dw_fold_h_k<MB>, dim3(kC * kC / 16), dim3(256), 0, stream, parts, partial, grad_w2, wd);
  const int64_t per_roi = static_cast<int64_t>(m) * s;
  if (per_roi <= kPtMax && n <= kPtMaxN) {   // grad_point of a RoI inside one workgroup
    const int len = static_cast<int>(next_pow2(static_cast<uint64_t>(per_roi)));
    if (dtype == FV2P_DT_F16)
      hipLaunchKernelGGL(sa_grid_points_h_k<MH>, dim3(rois), dim3(512), 0, stream, n, static_cast<int>(per_roi), len, idx, rows, static_cast<u16*>(grad_point));
    else
      hipLaunchKernelGGL(sa_grid_points_h_k<MB>, dim3(rois), dim3(512), 0, stream, n, static_cast<int>(per_roi), len, idx, rows, static_cast<u16*>(grad_point));
    FV2P_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL(sa_grid_entries_h_k, dim3(static_cast<unsigned>(ceil_div(entries, 256))), dim3(256), 0, stream, entries, n, per_roi, idx, dst);
  FV2P_LAUNCH_CHECK();
  return scatter_add_h(entries, kC, static_cast<int64_t>(rois) * n, dst, nullptr, nullptr, rows, 1, grad_point, dtype, sws, sb, stream);
}
