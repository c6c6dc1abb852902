// Fused grid set-abstraction of the RoI head (A11 consumers: PointnetSAModuleMSG as IoUGuidedRoIHead builds it,
// pcdet/models/roi_heads/iouguided_roi_head.py:52-76, 258-275; pcdet/ops/pointnet2/pointnet2_batch/pointnet2_modules.py:30-62), on fp32,
// float16 and bfloat16 rows: fv2p_sa_grid_fwd / _bwd / _bwd_gather and fv2p_sa_grid_fwd_h / _bwd_h (include/fv2p_ops.h).
//
// The reference materialises, per radius, the grouped tensor (R, 3 + C, M, S) — 1.39 GB at R = 384 RoIs, M = 216 grid centres,
// S = 32 samples — and runs its shared MLP (1x1 convs + ReLU) over it as plain GEMMs, then max-pools over the S samples.  With
// the first (linear) layer applied per POINT and per CENTRE beforehand (fv2p_harness/fv2p_model.py: sa_msg_grid), what is left
// per (centre i, sample s) is
//        h1 = relu(P[idx[i, s], :] - Q[i, :])          64 channels, P = per-point, Q = per-centre first-layer products
//        h2 = relu(W2 h1)                               second shared-MLP layer, 64 x 64
//        out[i, :] = max_s h2                           P (R, N, 64), Q / out (R, M, 64), S in {16, 32}
// and this file computes that without any grouped tensor: a wave gathers 16 sample rows, runs the 64 x 64 layer on MFMA against W2
// fragments resident in LDS, and reduces the maximum over the rows in registers.  The product is formed TRANSPOSED (h2^T = W2 h1^T):
// the 16 sample rows of a tile are the 16 lanes of a DPP row, and lane (row = l & 15, g = l >> 4), which supplied the channels
// 16 j + 4 g .. + 3 of its sample row as the B operand, receives the channels 16 b + 4 g .. + 3 of the same row in its accumulators,
// i.e. results have the operand layout and chain into the next product (backward: dh1^T = W2^T dh2^T) without any shuffle.
//
// The forward pass also stores, per centre and channel, WHICH sample attained the maximum (one byte; the first one in sample
// order, as the reference's F.max_pool2d does, pointnet2_modules.py:57-59, so ties between repeated indices go to the earliest slot;
// 255 = the maximum is 0, no gradient).  Backward recomputes h1 only (a gather and a subtraction) and routes d out to that sample.
// Rounds 1-2 stored nothing but `out` and recomputed h2 to find the maxima again: half of the backward pass's MFMA work, twice.
//
// ONE source for the three storage formats (F32, MH = float16, MB = bfloat16 below).  The forward kernel, the arg byte, the row
// reductions, the dW2 fold and the host-side checks are written once; a format supplies how a 16-channel block of a row is loaded,
// widened, rounded, stored and fed to the MFMA, and how W2 is staged.  Three things stay per format on purpose:
//   * where the forward issues its row loads (kLoadAhead): the 16-bit formats load all tiles' rows up front; fp32, whose rows are
//     twice as wide (32 more VGPRs for a second tile in flight), loads each tile's rows inside the tile loop;
//   * the index guard (kGuard): 16-bit, an index outside [0, N) reads as a row of zeros (h1 = relu(-Q)), is never dereferenced, and
//     backward drops its dh1 entry; fp32 requires indices in range and guards nothing - its backward (246 / 248 of 256 VGPRs at
//     S = 32) has no register for a guard, and forward and backward must agree;
//   * the backward ALGORITHM: two kernels, described in front of each.
// fp32: rows are 256 B, one float4 per lane and 16-channel block; 64 v_mfma_f32_16x16x4_f32 per tile of 16 samples against 16 KB of
// W2 fragments.
//
// 16-bit: P, Q, out and every gradient are stored in ONE 16-bit format T; W2 (64, 64) is T (wd != 0) or fp32 (wd == 0: the master
// weight an autocast caller has).  fp32 weights are rounded to T on their way into LDS - the bits of W2.to(T); no 16-bit copy exists
// in memory - and no fp32 image of P, Q, out or a gradient is made anywhere.  Arithmetic (the contract of tests/test_sa_half_gpu.py):
//   h1      = RNE_T(max(float(P) - float(Q), 0))    fp32 subtraction of the widened values, rounded once: the MFMA operand
//   a[s][o] = sum_c W2r[o][c] h1[s][c]              fp32 accumulators of v_mfma_f32_16x16x32_{f16,bf16}; a product of two T values is exact
//   out     = RNE_T(max(0, max_s a[s][o]))          the maximum over the fp32 accumulators, rounded once at the store
//   arg     = the first sample in sample order whose fp32 accumulator equals the maximum; 255 where the maximum is 0
// The 16x16x32 MFMA wants 8 contraction indices per lane and K step; the order of K inside an MFMA is free as long as A and B agree, so
// K index (step ks, g, j) stands for channel 32 ks + 16 (j >> 2) + 4 g + (j & 3): a lane's B operand is then the SAME 16 channels
// 16 b + 4 g + e it receives results for - four 8-byte loads of a 128-byte row, four lanes covering 32 contiguous bytes - and results
// chain into the next product and meet the mask [h1 > 0] without a shuffle.  The W2 (forward) and W2^T (backward) fragments are staged
// in LDS in that permutation, 8 KB, one 16-byte read per lane, block and K step.  8 MFMAs per tile of 16 samples instead of fp32's 64.
// Backward routes the 16-bit values of grad_out to the sample arg names (dh2, exact), and gives
//   dh1         = (W2r^T dh2) [h1 > 0]              16-bit MFMA, fp32 accumulators
//   grad_centre = -sum_s dh1                        fp32 sum over the tiles, then over the DPP row in a fixed order; one rounding
//   grad_point  : every (centre, sample) row of dh1 is rounded to T and STAGED IN 16 BITS in the workspace (one more rounding per addend:
//                 u_s = u in the tests' bound), then summed per point in fp32 in a fixed order and rounded once: by sa_grid_points_h_k
//                 up to 8192 samples per RoI (the head has 3456 / 6912), beyond that by scatter_add_h in the association of
//                 fv2p_scatter_add.  No atomics, no sums in LDS, no dP tile, hence no limit on N; the deterministic switch changes nothing.
//   grad_w2[o][c] = sum_{r,i,s} dh2[o] h1[c]        sample rows are the K dimension: both tiles go through LDS transposed ([channel][sample
//                 row], wave-private), one K = 32 step per centre (an S = 16 centre fills half of it, the other half stays zero); fp32 partial
//                 tile per workgroup (the four waves folded as (w0 + w2) + (w1 + w3)), the partials folded in a fixed order by
//                 sa_grid_dw_fold_k and written in W2's dtype: one rounding for a 16-bit weight, none for fp32.
// Every 16-bit result has the same bits from run to run and on any stream.
#include <initializer_list>
#include <type_traits>
#include "common.hpp"
#include "dt16.hpp"

namespace fv2p {
namespace {

using f32x4 = float __attribute__((ext_vector_type(4)));
using f16x8 = _Float16 __attribute__((ext_vector_type(8)));
using bf16x8 = __bf16 __attribute__((ext_vector_type(8)));

constexpr int kC = 64;             // channels of both layers
constexpr int kFwdCentres = 16;    // centres per workgroup, forward

// Reductions over the 16 lanes of a DPP row (= the 16 sample rows of a tile; lanes sharing l / 16 hold the same channels), 8 or 16
// values at a time, in four steps: quad_perm xor-1, xor-2, row_half_mirror, row_mirror.  Every lane of the row ends with the row's
// result, and the association is the same in every lane and every launch.
// The maximum (both forward kernels) and the 8-value sum (fp32 backward) are ONE asm statement each in step-major order: the DPP read
// of a value is then N instructions behind the write it depends on (the two wait states a DPP operand needs are covered by the other
// values' instructions) and the compiler cannot slip a register copy in front of a step.  The preprocessor assembles the text, each
// step written once.  The form on __builtin_amdgcn_update_dpp below compiles to four instructions per value and step (zero,
// v_mov_b32_dpp, canonicalise, operate) where the asm is one: with it the fp32 forward lost 9 - 14 %, and the fp32 backward's S = 16
// instances gained 1 - 2 VGPRs.  The 16-value sum (16-bit backward, once per centre beside 16 - 32 MFMAs) stays on the builtin: as asm
// it costs that kernel 1 - 6 VGPRs.  Figures: profiles/refactor_sa.txt.
#define FV2P_DPP1(op, k, ctrl) op " %" #k ", %" #k ", %" #k " " ctrl " row_mask:0xf bank_mask:0xf\n\t"
#define FV2P_DPP8(op, ctrl) \
  FV2P_DPP1(op, 0, ctrl) FV2P_DPP1(op, 1, ctrl) FV2P_DPP1(op, 2, ctrl) FV2P_DPP1(op, 3, ctrl) FV2P_DPP1(op, 4, ctrl) FV2P_DPP1(op, 5, ctrl) FV2P_DPP1(op, 6, ctrl) FV2P_DPP1(op, 7, ctrl)
#define FV2P_DPP16(op, ctrl) \
  FV2P_DPP8(op, ctrl) FV2P_DPP1(op, 8, ctrl) FV2P_DPP1(op, 9, ctrl) FV2P_DPP1(op, 10, ctrl) FV2P_DPP1(op, 11, ctrl) FV2P_DPP1(op, 12, ctrl) FV2P_DPP1(op, 13, ctrl) FV2P_DPP1(op, 14, ctrl) FV2P_DPP1(op, 15, ctrl)
#define FV2P_ROW16(REP, op) "s_nop 1\n\t" REP(op, "quad_perm:[1,0,3,2]") REP(op, "quad_perm:[2,3,0,1]") REP(op, "row_half_mirror") REP(op, "row_mirror") "s_nop 1"
#define FV2P_V8(v) "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7])
#define FV2P_V16(v) FV2P_V8(v), "+v"(v[8]), "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]), "+v"(v[14]), "+v"(v[15])
__device__ __forceinline__ void row16_max_n(float (&v)[16]) { asm volatile(FV2P_ROW16(FV2P_DPP16, "v_max_f32_dpp") : FV2P_V16(v)); }
__device__ __forceinline__ void row16_sum_n(float (&v)[8]) { asm volatile(FV2P_ROW16(FV2P_DPP8, "v_add_f32_dpp") : FV2P_V8(v)); }
template <int CTRL>
__device__ __forceinline__ void row16_sum_step(float (&v)[16]) {
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = v[k] + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[k]), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ void row16_sum_n(float (&v)[16]) {
  row16_sum_step<0xB1>(v); row16_sum_step<0x4E>(v); row16_sum_step<0x141>(v); row16_sum_step<0x140>(v);
}

// ------------------------------------------------------------------ storage formats -------------------------------------------
// A format F supplies: elem (the element in memory), Blk (a lane's four channels 16 b + 4 g .. + 3 of a row as loaded), Wide (the same
// four in fp32, for Q), load / widen4 / relu_sub / positive ([h1 > 0] on the MFMA operand) / store4 (four fp32 results -> memory, ONE
// rounding), stage_w (W2, or W2^T with TR, as the A operand of D = A X^T in LDS; W32: the weight is fp32 in memory), mma64
// (acc[b] += A-fragments(lds)[b] * x, x[j] = this lane's Blk of channel block j of its sample row), store_w (one element of grad_w2),
// and the two placement switches of the header: kGuard, kLoadAhead.
struct F32 {
  using elem = float;
  using Blk = float4;
  using Wide = float4;
  static constexpr bool kGuard = false, kLoadAhead = false;
  static constexpr int kFragElems = 16 * 64 * 4;   // 16 KB
  static __device__ __forceinline__ Blk load(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ void widen4(Blk v, Wide& q) { q = v; }
  static __device__ __forceinline__ Blk relu_sub(Blk p, Wide q) {
    return make_float4(fmaxf(p.x - q.x, 0.f), fmaxf(p.y - q.y, 0.f), fmaxf(p.z - q.z, 0.f), fmaxf(p.w - q.w, 0.f));
  }
  static __device__ __forceinline__ bool positive(Blk h, int e) {
    const float hv[4] = {h.x, h.y, h.z, h.w};
    return hv[e] > 0.f;
  }
  static __device__ __forceinline__ void store4(float* p, float a, float b, float c, float d) { *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d); }
  static __device__ __forceinline__ void store_w(void* w, int e, float v, int) { static_cast<float*>(w)[e] = v; }
  // frag[b][j][lane] (float4) = A[16 b + lane % 16][16 j + 4 (lane / 16) .. + 3]
  template <bool W32, bool TR>
  static __device__ __forceinline__ void stage_w(const void* __restrict__ w, float* __restrict__ lds) {
    const float* a = static_cast<const float*>(w);
    for (int e = threadIdx.x; e < 16 * 64; e += 256) {
      const int lane = e & 63, bj = e >> 6, b = bj >> 2, j = bj & 3;
      const int row = 16 * b + (lane & 15), col = 16 * j + 4 * (lane >> 4);
      static_assert(!TR, "the fp32 backward stages its half of W2^T itself");
      *reinterpret_cast<float4*>(lds + e * 4) = *reinterpret_cast<const float4*>(a + row * kC + col);
    }
  }
  static __device__ __forceinline__ void mma64(const float* __restrict__ frag, int lane, const Blk (&x)[4], f32x4 (&acc)[4]) {
    // j outer, the four accumulator blocks inner: consecutive MFMAs belong to different dependency chains
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float4 a[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) a[b] = *reinterpret_cast<const float4*>(frag + ((b * 4 + j) * 64 + lane) * 4);
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[b].x, x[j].x, acc[b], 0, 0, 0);
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[b].y, x[j].y, acc[b], 0, 0, 0);
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[b].z, x[j].z, acc[b], 0, 0, 0);
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[b].w, x[j].w, acc[b], 0, 0, 0);
    }
  }
};

struct CvtH : H16 {
  static __device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};
struct CvtB : B16 {
  // gfx950 converts in hardware (v_cvt_pk_bf16_f32: nearest even, NaN stays a quiet NaN): the bits of B16::round
  static __device__ __forceinline__ u16 round(float v) { return __builtin_bit_cast(u16, static_cast<__bf16>(v)); }
  static __device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};
__device__ __forceinline__ unsigned elem16(uint2 v, int e) { return ((e < 2 ? v.x : v.y) >> (16 * (e & 1))) & 0xffffu; }

template <class T>   // T: widen, round (also what Row16<F, 8> asks of F) and mfma
struct Fmt16 : T {
  using elem = u16;
  using Blk = uint2;
  using Wide = float[4];
  static constexpr bool kGuard = true, kLoadAhead = true;
  static constexpr int kFragElems = 8 * 64 * 8;   // 8 KB
  static __device__ __forceinline__ Blk load(const u16* p) { return *reinterpret_cast<const uint2*>(p); }
  static __device__ __forceinline__ void widen4(Blk v, float (&f)[4]) {
    f[0] = T::widen(static_cast<u16>(v.x & 0xffffu)); f[1] = T::widen(static_cast<u16>(v.x >> 16));
    f[2] = T::widen(static_cast<u16>(v.y & 0xffffu)); f[3] = T::widen(static_cast<u16>(v.y >> 16));
  }
  static __device__ __forceinline__ Blk round4(float a, float b, float c, float d) {
    return make_uint2(static_cast<unsigned>(T::round(a)) | (static_cast<unsigned>(T::round(b)) << 16),
                      static_cast<unsigned>(T::round(c)) | (static_cast<unsigned>(T::round(d)) << 16));
  }
  // h1 = RNE_T(max(p - q, 0)) for four channels
  static __device__ __forceinline__ Blk relu_sub(Blk p, const float (&q)[4]) {
    float f[4];
    widen4(p, f);
    return round4(fmaxf(f[0] - q[0], 0.f), fmaxf(f[1] - q[1], 0.f), fmaxf(f[2] - q[2], 0.f), fmaxf(f[3] - q[3], 0.f));
  }
  static __device__ __forceinline__ bool positive(Blk h, int e) { return (elem16(h, e) & 0x7fffu) != 0u; }   // on the rounded h1 (never negative; -0 counts as 0)
  static __device__ __forceinline__ void store4(u16* p, float a, float b, float c, float d) { *reinterpret_cast<uint2*>(p) = round4(a, b, c, d); }
  static __device__ __forceinline__ void store_w(void* w, int e, float v, int wd) {   // fp32 as it is (wd == 0) or rounded once
    if (wd) static_cast<u16*>(w)[e] = T::round(v);
    else static_cast<float*>(w)[e] = v;
  }
  template <bool W32>
  static __device__ __forceinline__ unsigned w_at(const void* __restrict__ w, int o, int c) {
    if constexpr (W32) return T::round(static_cast<const float*>(w)[o * kC + c]);
    else return static_cast<const u16*>(w)[o * kC + c];
  }
  // frag[b][ks][lane] (8 elements) = A[16 b + lane % 16][k], k the permuted channel 32 ks + 16 (j >> 2) + 4 (lane / 16) + (j & 3), j = 0..7
  template <bool W32, bool TR>
  static __device__ __forceinline__ void stage_w(const void* __restrict__ w, u16* __restrict__ lds) {
    for (int e = threadIdx.x; e < 8 * 64; e += 256) {
      const int lane = e & 63, ks = (e >> 6) & 1, b = e >> 7;
      const int rw = 16 * b + (lane & 15), g = lane >> 4;
      unsigned wv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k0 = 32 * ks + 16 * (i >> 1) + 4 * g + 2 * (i & 1);
        const unsigned lo = TR ? w_at<W32>(w, k0, rw) : w_at<W32>(w, rw, k0);
        const unsigned hi = TR ? w_at<W32>(w, k0 + 1, rw) : w_at<W32>(w, rw, k0 + 1);
        wv[i] = lo | (hi << 16);
      }
      *reinterpret_cast<uint4*>(lds + e * 8) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
    }
  }
  static __device__ __forceinline__ void mma64(const u16* __restrict__ frag, int lane, const Blk (&x)[4], f32x4 (&acc)[4]) {
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
};
using MH = Fmt16<CvtH>;
using MB = Fmt16<CvtB>;

// Row `src` of a RoI's points as this lane reads it: blk(b) = its channels 16 b + 4 g .. + 3.  kGuard: outside [0, n) the row reads as
// zeros and is never dereferenced
template <class F>
struct RowAt {
  const typename F::elem* p;
  bool ok;
  __device__ __forceinline__ RowAt(const typename F::elem* Pr, int src, int n, int g) {
    ok = !F::kGuard || static_cast<unsigned>(src) < static_cast<unsigned>(n);
    p = Pr + static_cast<long long>(ok ? src : 0) * kC + 4 * g;
  }
  __device__ __forceinline__ typename F::Blk blk(int b) const {
    if constexpr (F::kGuard) return ok ? F::load(p + 16 * b) : make_uint2(0u, 0u);
    else return F::load(p + 16 * b);
  }
};

// ------------------------------------------------------------------ forward ---------------------------------------------------
// grid (ceil(M / 16), R), block 256: wave w handles centres 16 * blockIdx.x + w, w + 4, ...   TILES = S / 16
template <class F, int TILES, bool W32>
__global__ __launch_bounds__(256) void sa_grid_fwd_k(int n, int m, const typename F::elem* __restrict__ P, const typename F::elem* __restrict__ Q,
                                                     const int* __restrict__ idx, const void* __restrict__ W2, typename F::elem* __restrict__ out,
                                                     unsigned char* __restrict__ arg) {
  using Blk = typename F::Blk;
  __shared__ __attribute__((aligned(16))) typename F::elem wfrag[F::kFragElems];
  constexpr int s = 16 * TILES;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, g = lane >> 4;
  const int r = blockIdx.y;
  F::template stage_w<W32, false>(W2, wfrag);
  __syncthreads();
  const typename F::elem* Pr = P + static_cast<long long>(r) * n * kC;
  for (int ci = wave; ci < kFwdCentres; ci += 4) {
    const int i = blockIdx.x * kFwdCentres + ci;
    if (i >= m) break;
    const long long ctr = static_cast<long long>(r) * m + i;
    int src[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t) src[t] = idx[ctr * s + 16 * t + row];
    Blk qraw[4], praw[F::kLoadAhead ? TILES : 1][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) qraw[b] = F::load(Q + ctr * kC + 16 * b + 4 * g);
    if constexpr (F::kLoadAhead) {
#pragma unroll
      for (int t = 0; t < TILES; ++t) {
        const RowAt<F> at(Pr, src[t], n, g);
#pragma unroll
        for (int b = 0; b < 4; ++b) praw[t][b] = at.blk(b);
      }
    }
    typename F::Wide qf[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) F::widen4(qraw[b], qf[b]);
    float best[16];
    uint32_t late = 0;   // bit 4 b + e: this lane's best value of that channel came from the second tile
#pragma unroll
    for (int k = 0; k < 16; ++k) best[k] = 0.f;   // relu output: the maximum is >= 0
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      if constexpr (!F::kLoadAhead) {
        const RowAt<F> at(Pr, src[t], n, g);
#pragma unroll
        for (int b = 0; b < 4; ++b) praw[0][b] = at.blk(b);
      }
      Blk x[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) x[b] = F::relu_sub(praw[F::kLoadAhead ? t : 0][b], qf[b]);
      f32x4 acc[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
      F::mma64(wfrag, lane, x, acc);
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (t != 0 && acc[b][e] > best[4 * b + e]) late |= 1u << (4 * b + e);   // strict: the earlier sample keeps a tie
          best[4 * b + e] = fmaxf(best[4 * b + e], acc[b][e]);
        }
    }
    // lane (row, g) holds channels 16 b + 4 g + e of sample row `row`: maximum over the 16 lanes of the DPP row
    __builtin_amdgcn_sched_barrier(0);   // the tile loop is scheduled on its own: with the reduction's 16 tied registers in its region the 16-bit S = 32 instances need 98 VGPRs, two more than five waves per SIMD allow
    float flat[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) flat[k] = best[k];
    row16_max_n(flat);
    if (row == 0) {
      typename F::elem* o = out + ctr * kC + 4 * g;
#pragma unroll
      for (int b = 0; b < 4; ++b) F::store4(o + 16 * b, flat[4 * b], flat[4 * b + 1], flat[4 * b + 2], flat[4 * b + 3]);
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

// ------------------------------------------------------------------ backward, fp32 --------------------------------------------
// Produces dP (scatter-add into an LDS tile per RoI and 32-channel half, flushed once; or, DET, dh1 rows for the fixed-order
// fv2p_scatter_add), dQ (row sums, direct stores) and dW2 (MFMA over the sample rows after an LDS transpose; one partial tile per
// workgroup, summed by a second launch).  grid (2, R): workgroup (h, r) owns the channel half h of dP / dQ (channels 32 h .. 32 h + 31)
// and the row half h of dW2 (output channels c' in the same range) of RoI r; block 512 (256), wave w takes centres w, w + 8 (4), ...
constexpr int kSaTs = 72;   // row stride of the transpose tiles (floats): 64 + 8, conflict-light both ways
constexpr int kSaDp = 33;   // row stride of the dP tile (floats): odd, so the scatter's rows (arbitrary points) spread over all LDS banks —
                            // with 32 every row starts on bank 0 or 32 and a wave's 64 adds fall on 8 banks
// kSaBwdWaves = 8 where the dP tile leaves room for eight waves' transpose tiles (n <= 589), two per SIMD: one wave's gathers, LDS
// atomics and transposes run beside the other's MFMAs (one workgroup per CU either way: the dP tile); 4 above that.
// DET (fv2p_sa_grid_bwd_gather): instead of the LDS atomics into the dP tile, every (centre, sample) row of dh1 is stored to
// dh1_rows[(r * m + i) * s + sample][64] (zeros included) and summed per point afterwards in the fixed order of fv2p_scatter_add.
template <int TILES, int kSaBwdWaves, bool DET>   // TILES = samples per centre / 16: register arrays below are indexed by compile-time tile numbers only
__global__ __launch_bounds__(kSaBwdWaves * 64) void sa_grid_bwd_k(int n, int m, const float* __restrict__ P, const float* __restrict__ Q,
                                                     const int* __restrict__ idx, const float* __restrict__ W2, const unsigned char* __restrict__ arg,
                                                     const float* __restrict__ dout, float* __restrict__ dP, float* __restrict__ dQ,
                                                     float* __restrict__ dW2_partial, float* __restrict__ dh1_rows) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* wtfrag = lds;                         // W2^T    as A operand (dh1^T = W2^T dh2^T), this half's two row blocks only: 8 KB
  float* tile = wtfrag + 8 * 64 * 4;           // per wave: two 16 x 72 transpose tiles (dh2, h1)
  float* dpt = tile + kSaBwdWaves * 2 * 16 * kSaTs;      // dP accumulator of this RoI and channel half: [n][kSaDp]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, g = lane >> 4;
  const int half = blockIdx.x, r = blockIdx.y;
  // fragments [bb][j][lane] of W2^T rows 32 half + 16 bb + lane % 16, columns 16 j + 4 (lane / 16) .. + 3
  for (int e = threadIdx.x; e < 8 * 64; e += kSaBwdWaves * 64) {
    const int l = e & 63, bj = e >> 6, bb = bj >> 2, j = bj & 3;
    const int rw = 32 * static_cast<int>(blockIdx.x) + 16 * bb + (l & 15), col = 16 * j + 4 * (l >> 4);
    *reinterpret_cast<float4*>(wtfrag + e * 4) = make_float4(W2[(col + 0) * kC + rw], W2[(col + 1) * kC + rw], W2[(col + 2) * kC + rw], W2[(col + 3) * kC + rw]);
  }
  if constexpr (!DET)
    for (int e = threadIdx.x; e < n * kSaDp; e += kSaBwdWaves * 64) dpt[e] = 0.f;
  __syncthreads();
  float* t_dh2 = tile + wave * 2 * 16 * kSaTs;
  float* t_h1 = t_dh2 + 16 * kSaTs;
  const float* Pr = P + static_cast<long long>(r) * n * kC;
  // dW2 rows c' = 32 half + 16 bb + ..., all 64 columns: 2 x 4 accumulator tiles, summed over every sample row this wave sees
  f32x4 dw[2][4];
#pragma unroll
  for (int bb = 0; bb < 2; ++bb)
#pragma unroll
    for (int bc = 0; bc < 4; ++bc) dw[bb][bc] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int s = TILES * 16;
  // A centre's inputs come from two dependent rounds of global loads (its sample list, then the rows the list names): ~2 x 2 us that
  // nothing covered while the centre's own work is 2 - 4 k clocks of matrix pipe - the round-3 kernel spent 13.8 k clocks per centre and
  // wave.  Now they are two centres deep in flight: while centre i multiplies, the rows / centre vector / arg bytes / gradient of centre
  // i + W and the sample list of centre i + 2 W are on their way (W = waves of the workgroup).  The prefetches are issued AFTER the
  // current centre's operands have been consumed into x[][], so that the wait in front of that use has only loads of the iteration
  // before to wait for.
  struct Staged { float4 qv[4], gd[4], praw[TILES][4]; uint32_t who[4]; int src[TILES]; };
  auto centre_of = [&](int i) { return static_cast<long long>(r) * m + (i < m ? i : m - 1); };   // past the end: the last centre again (never used)
  auto load_list = [&](int i, int (&src)[TILES]) {
    const int* id = idx + centre_of(i) * s;
#pragma unroll
    for (int t = 0; t < TILES; ++t) src[t] = id[16 * t + row];
  };
  auto load_rows = [&](int i, Staged& c) {   // c.src holds the list already
    const long long ctr = centre_of(i);
    const float* q = Q + ctr * kC + 4 * g;
    const unsigned char* am = arg + ctr * kC + 4 * g;
    const float* go = dout + ctr * kC + 4 * g;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c.qv[j] = *reinterpret_cast<const float4*>(q + 16 * j);
      c.who[j] = *reinterpret_cast<const uint32_t*>(am + 16 * j);
      c.gd[j] = *reinterpret_cast<const float4*>(go + 16 * j);
    }
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      const float* p = Pr + static_cast<long long>(c.src[t]) * kC + 4 * g;
#pragma unroll
      for (int j = 0; j < 4; ++j) c.praw[t][j] = F32::load(p + 16 * j);
    }
  };
  Staged cur, nxt;
  int list2[TILES];
  load_list(wave, cur.src);
  load_rows(wave, cur);
  load_list(wave + kSaBwdWaves, nxt.src);
  for (int i = wave; i < m; i += kSaBwdWaves) {
    uint32_t who[4];   // byte e of who[b]: the sample that attained the maximum of channel 16 b + 4 g + e (255: none)
    float4 gd[4];
    float4 x[TILES][4];
    int src[TILES];
#pragma unroll
    for (int b = 0; b < 4; ++b) { who[b] = cur.who[b]; gd[b] = cur.gd[b]; }
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      src[t] = cur.src[t];
#pragma unroll
      for (int j = 0; j < 4; ++j) x[t][j] = F32::relu_sub(cur.praw[t][j], cur.qv[j]);
    }
    __builtin_amdgcn_sched_barrier(0);   // the prefetches stay behind the use above
    load_rows(i + kSaBwdWaves, nxt);
    load_list(i + 2 * kSaBwdWaves, list2);
    __builtin_amdgcn_sched_barrier(0);
    // pass 2 per tile: dh2, dh1 = (W2^T dh2) * [h1 > 0], scatter / reduce, dW2 += dh2^T h1
    float dq[2][4];
#pragma unroll
    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
      for (int e = 0; e < 4; ++e) dq[bb][e] = 0.f;
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      float4 dh2[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float gv[4] = {gd[b].x, gd[b].y, gd[b].z, gd[b].w};
        float d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = ((who[b] >> (8 * e)) & 0xffu) == static_cast<uint32_t>(16 * t + row) ? gv[e] : 0.f;
        dh2[b] = make_float4(d[0], d[1], d[2], d[3]);
      }
      // dh1^T block bb of this half: channels 32 half + 16 bb + 4 g + e
      f32x4 d1[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 a0 = *reinterpret_cast<const float4*>(wtfrag + ((0 * 4 + j) * 64 + lane) * 4);
        const float4 a1 = *reinterpret_cast<const float4*>(wtfrag + ((1 * 4 + j) * 64 + lane) * 4);
        d1[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, dh2[j].x, d1[0], 0, 0, 0);
        d1[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, dh2[j].x, d1[1], 0, 0, 0);
        d1[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, dh2[j].y, d1[0], 0, 0, 0);
        d1[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, dh2[j].y, d1[1], 0, 0, 0);
        d1[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, dh2[j].z, d1[0], 0, 0, 0);
        d1[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, dh2[j].z, d1[1], 0, 0, 0);
        d1[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, dh2[j].w, d1[0], 0, 0, 0);
        d1[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, dh2[j].w, d1[1], 0, 0, 0);
      }
#pragma unroll
      for (int bb = 0; bb < 2; ++bb) {
        const float4 h = half ? x[t][2 + bb] : x[t][bb];   // (a runtime index would push the array into scratch)
        const float hv[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = hv[e] > 0.f ? d1[bb][e] : 0.f;
          dq[bb][e] += v;
          if constexpr (DET) dh1_rows[((static_cast<long long>(r) * m + i) * s + 16 * t + row) * kC + 32 * half + 16 * bb + 4 * g + e] = v;
          else if (v != 0.f) atomicAdd(&dpt[src[t] * kSaDp + 16 * bb + 4 * g + e], v);
        }
      }
      // dW2[c'][c] += sum_rows dh2[row][c'] h1[row][c]: rows become the K dimension -> transpose both tiles through LDS
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        *reinterpret_cast<float4*>(t_h1 + row * kSaTs + 16 * b + 4 * g) = x[t][b];
        if ((b >> 1) == half) *reinterpret_cast<float4*>(t_dh2 + row * kSaTs + 16 * (b & 1) + 4 * g) = dh2[b];
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's own LDS writes (tiles are private to the wave)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {       // K step: sample rows 4 ks + g
        float a[2], bcol[4];
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) a[bb] = t_dh2[(4 * ks + g) * kSaTs + 16 * bb + row];       // A[m = c' % 16][k = row]
#pragma unroll
        for (int bc = 0; bc < 4; ++bc) bcol[bc] = t_h1[(4 * ks + g) * kSaTs + 16 * bc + row];      // B[k = row][n = c % 16]
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
          for (int bc = 0; bc < 4; ++bc) dw[bb][bc] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[bb], bcol[bc], dw[bb][bc], 0, 0, 0);
      }
    }
    // dQ[i][c] = - sum over the centre's samples of dh1 (the 16 lanes of the DPP row), this half's 32 channels
    float* dqo = dQ + (static_cast<long long>(r) * m + i) * kC + 32 * half + 4 * g;
    float flat[8];
#pragma unroll
    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
      for (int e = 0; e < 4; ++e) flat[4 * bb + e] = dq[bb][e];
    row16_sum_n(flat);
    if (row == 0) {
      *reinterpret_cast<float4*>(dqo) = make_float4(-flat[0], -flat[1], -flat[2], -flat[3]);
      *reinterpret_cast<float4*>(dqo + 16) = make_float4(-flat[4], -flat[5], -flat[6], -flat[7]);
    }
    cur = nxt;
#pragma unroll
    for (int t = 0; t < TILES; ++t) nxt.src[t] = list2[t];
  }
  __syncthreads();
  // flush dP (each (RoI, half) tile is owned by this workgroup: plain stores)
  float* dpo = dP + static_cast<long long>(r) * n * kC + 32 * half;
  for (int e = threadIdx.x; e < (DET ? 0 : n * 8); e += kSaBwdWaves * 64) {
    const int pt = e >> 3, c4 = (e & 7) * 4;
    const float* t4 = dpt + pt * kSaDp + c4;
    *reinterpret_cast<float4*>(dpo + static_cast<long long>(pt) * kC + c4) = make_float4(t4[0], t4[1], t4[2], t4[3]);
  }
  // dW2 partial of this workgroup: the waves' accumulators summed through LDS (the transpose tiles are free now)
  __syncthreads();
  float* buf = lds;    // fragments + tiles (8 + 74 KB, all waves are past them): room for 8 waves x 2 x 4 x 64 x 4 floats = 64 KB
#pragma unroll
  for (int bb = 0; bb < 2; ++bb)
#pragma unroll
    for (int bc = 0; bc < 4; ++bc)
      *reinterpret_cast<f32x4*>(buf + (((wave * 2 + bb) * 4 + bc) * 64 + lane) * 4) = dw[bb][bc];
  __syncthreads();
  // accumulator (bb, bc) of lane l holds dW2[32 half + 16 bb + 4 (l / 16) + e][16 bc + l % 16]
  float* dwo = dW2_partial + (static_cast<long long>(r) * 2 + half) * 32 * kC;
  for (int e = threadIdx.x; e < 2 * 4 * 64 * 4; e += kSaBwdWaves * 64) {
    const int comp = e & 3, l = (e >> 2) & 63, bc = (e >> 8) & 3, bb = e >> 10;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < kSaBwdWaves; ++w) v += buf[(((w * 2 + bb) * 4 + bc) * 64 + l) * 4 + comp];
    dwo[(16 * bb + 4 * (l >> 4) + comp) * kC + 16 * bc + (l & 15)] = v;
  }
}

// ------------------------------------------------------------------ backward, 16-bit ------------------------------------------
// grid (ceil(M / 64), R), block 256: wave w takes centres 64 * blockIdx.x + w, w + 4, ...  LDS: the W2^T fragments (8 KB) and per wave
// two transposed tiles [64 channels][kLd] (dh2, h1: 10 KB), 48 KB; the fold of the waves' dW2 accumulators reuses it.
constexpr int kBwdCentres = 64;    // centres per workgroup (one fp32 dW2 partial tile each)
constexpr int kLd = 40;            // row stride of the transposed tiles in elements: 32 sample rows + 8 (80-byte rows, 16-byte aligned)
constexpr int kBwdLds = 8 * 64 * 8 * 2 + 4 * 2 * kC * kLd * 2;

template <class F, int TILES, bool W32>
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
  F::template stage_w<W32, true>(W2, wtfrag);
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
      qraw[b] = F::load(Q + ctr * kC + 16 * b + 4 * g);
      graw[b] = F::load(dout + ctr * kC + 16 * b + 4 * g);
      who[b] = *reinterpret_cast<const uint32_t*>(arg + ctr * kC + 16 * b + 4 * g);
    }
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      const bool ok = static_cast<unsigned>(src[t]) < static_cast<unsigned>(n);
      const u16* p = Pr + static_cast<long long>(ok ? src[t] : 0) * kC + 4 * g;
#pragma unroll
      for (int b = 0; b < 4; ++b) praw[t][b] = ok ? F::load(p + 16 * b) : make_uint2(0u, 0u);
    }
    typename F::Wide qf[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) F::widen4(qraw[b], qf[b]);
    float dq[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) dq[k] = 0.f;
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
      uint2 x[4], dh2[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        x[b] = F::relu_sub(praw[t][b], qf[b]);
        unsigned d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = ((who[b] >> (8 * e)) & 0xffu) == static_cast<uint32_t>(16 * t + row) ? elem16(graw[b], e) : 0u;
        dh2[b] = make_uint2(d[0] | (d[1] << 16), d[2] | (d[3] << 16));
      }
      f32x4 d1[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) d1[b] = f32x4{0.f, 0.f, 0.f, 0.f};
      F::mma64(wtfrag, lane, dh2, d1);   // dh1^T = W2^T dh2^T: channels 16 b + 4 g + e of this lane's sample row
      u16* ro = dh1_rows + ((ctr * s + 16 * t + row) * kC + 4 * g);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = F::positive(x[b], e) ? d1[b][e] : 0.f;
          dq[4 * b + e] += v[e];
        }
        F::store4(ro + 16 * b, v[0], v[1], v[2], v[3]);
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
        for (int bc = 0; bc < 4; ++bc) dw[bo][bc] = F::mfma(a[bo], bf[bc], dw[bo][bc]);
    }
    __builtin_amdgcn_wave_barrier();
    // dQ[i][c] = - sum over the centre's samples of dh1 (the 16 lanes of the DPP row)
    row16_sum_n(dq);
    if (row == 0) {
      u16* dqo = dQ + ctr * kC + 4 * g;
#pragma unroll
      for (int b = 0; b < 4; ++b) F::store4(dqo + 16 * b, -dq[4 * b], -dq[4 * b + 1], -dq[4 * b + 2], -dq[4 * b + 3]);
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

// dW2[c'][c] = sum of the partial tiles: the tiles are one [parts][64 * 64] matrix, the result its column sums.  A workgroup owns 16
// columns; its 256 threads are 16 row groups x 16 columns, a thread adds the rows rg, rg + 16, ... in ascending order and the 16 group
// sums are added in group order: a fixed association (deterministic).  (One thread per column walking all the rows, the round-3 form,
// took 98 us at 384 RoIs - a fifth of the backward kernel beside it.)  Written in W2's dtype (F::store_w).
template <class F>
__global__ __launch_bounds__(256) void sa_grid_dw_fold_k(int parts, const float* __restrict__ partial, void* __restrict__ dW2, int wd) {
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
    F::store_w(dW2, blockIdx.x * 16 + threadIdx.x, v, wd);
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
__global__ void sa_grid_entries_k(int64_t entries, int n, int64_t per_roi, const int* __restrict__ idx, int* __restrict__ dst) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= entries) return;
  const int i = idx[e];
  dst[e] = i >= 0 && i < n ? static_cast<int>((e / per_roi) * n + i) : -1;
}

// ------------------------------------------------------------------ host ------------------------------------------------------
bool shapes_ok(int rois, int n, int m, int s, int c) {
  return rois >= 1 && rois <= 65535 && n >= 1 && m >= 1 && c == kC && (s == 16 || s == 32);
}
int chunks_of(int m) { return static_cast<int>(ceil_div(m > 0 ? m : 1, kBwdCentres)); }

// the argument checks the entry points share (`who`: the message prefix); 0 or the error code
int none_null(const char* who, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs) FV2P_REQUIRE(p, FV2P_EINVAL, "%s: null pointer", who);
  return 0;
}
int all_aligned16(const char* who, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs) FV2P_REQUIRE(aligned16(p), FV2P_EINVAL, "%s: rows must be 16-byte aligned", who);
  return 0;
}
int dtypes_ok(const char* who, int dtype, int wd) {
  FV2P_DT16_OK(who, dtype);
  FV2P_REQUIRE(wd == 0 || wd == dtype, FV2P_EINVAL, "%s: w2 is fp32 (wd 0) or has the rows' dtype, got wd %d beside dtype %d", who, wd, dtype);
  return 0;
}
int counts_fit(const char* who, int rois, int n, int m, int s) {   // row numbers of the staged dh1 rows and of grad_point are ints
  FV2P_REQUIRE(static_cast<int64_t>(rois) * m * s < (1ll << 31) && static_cast<int64_t>(rois) * n < (1ll << 31) - 1, FV2P_ELIMIT, "%s: too many samples", who);
  return 0;
}

// Workspace of the backward passes that stage dh1 rows (fv2p_sa_grid_bwd_gather: fp32 rows; fv2p_sa_grid_bwd_h: 16-bit rows): `parts` fp32
// dW2 partial tiles, the entries' destination rows, the staged rows, the scatter-add's own workspace.  One walk serves the *_ws_bytes
// query (Sizer) and the call (Carver).
struct GatherWs {
  float* partial;
  int* dst;
  void *rows, *sws;
  size_t sws_bytes;
  template <class Taker>
  GatherWs(Taker&& tk, size_t parts, int64_t entries, size_t elem_bytes) {
    partial = tk.template take<float>(parts * kC * kC);
    dst = tk.template take<int>(static_cast<size_t>(entries));
    rows = tk.template take<char>(static_cast<size_t>(entries) * kC * elem_bytes);
    sws_bytes = fv2p_scatter_add_ws_bytes(entries, kC);
    sws = tk.template take<char>(sws_bytes);
  }
};
size_t gather_ws_bytes(size_t parts, int rois, int m, int s, size_t elem_bytes) {
  Sizer sz;
  GatherWs(sz, parts, static_cast<int64_t>(rois > 0 ? rois : 1) * (m > 0 ? m : 1) * (s > 0 ? s : 1), elem_bytes);
  return sz.bytes();
}

// (dtype, S, wd) -> fn(format, TILES, W32) with the three as types: the one place that names the instances of a 16-bit kernel
template <class Fn>
void with_tiles(int s, Fn&& fn) {
  if (s == 16) fn(std::integral_constant<int, 1>{});
  else fn(std::integral_constant<int, 2>{});
}
template <class Fn>
void with_format16(int dtype, Fn&& fn) {
  if (dtype == FV2P_DT_F16) fn(MH{});
  else fn(MB{});
}
template <class Fn>
void with_instance16(int dtype, int s, int wd, Fn&& fn) {
  with_format16(dtype, [&](auto f) {
    with_tiles(s, [&](auto tiles) {
      if (wd) fn(f, tiles, std::false_type{});
      else fn(f, tiles, std::true_type{});
    });
  });
}

template <class F, int TILES, bool W32>
void launch_fwd(const void* P, const void* Q, const int* idx, const void* w2, int rois, int n, int m, void* out, unsigned char* arg, hipStream_t st) {
  using E = typename F::elem;
  hipLaunchKernelGGL((sa_grid_fwd_k<F, TILES, W32>), dim3(static_cast<unsigned>(ceil_div(m, kFwdCentres)), rois), dim3(256), 0, st, n, m,
                     static_cast<const E*>(P), static_cast<const E*>(Q), idx, w2, static_cast<E*>(out), arg);
}

// dh1_rows == nullptr: the LDS-atomic kernel (fv2p_sa_grid_bwd); otherwise the DET one, which leaves grad_point to the caller
template <bool DET>
int sa_grid_bwd_launch(const float* per_point, const float* per_centre, const int* idx, const float* w2, const unsigned char* arg,
                       const float* grad_out, int rois, int n, int m, int s, float* grad_point, float* grad_centre, float* grad_w2,
                       float* partial, float* dh1_rows, hipStream_t stream) {
  auto lds_of = [&](int waves) { return (8 * 64 * 4 + static_cast<size_t>(waves) * 2 * 16 * kSaTs + static_cast<size_t>(n) * kSaDp) * sizeof(float); };
  const int waves = lds_of(8) <= 160 * 1024 ? 8 : 4;
  const size_t lds = lds_of(waves);
  static bool roomy[4] = {false, false, false, false};   // per kernel instance: the dynamic-LDS limit is raised once
  bool& raised = roomy[(s == 32 ? 2 : 0) + (waves == 8 ? 1 : 0)];   // (one table per DET instance of this function)
  auto launch = [&](auto kernel) -> int {
    if (lds > 48 * 1024 && !raised) {
      FV2P_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      raised = true;
    }
    hipLaunchKernelGGL(kernel, dim3(2, rois), dim3(waves * 64), lds, stream, n, m, per_point, per_centre, idx, w2, arg, grad_out, grad_point, grad_centre, partial,
                       dh1_rows);
    return 0;
  };
  int rc = 0;
  with_tiles(s, [&](auto tiles) { rc = waves == 8 ? launch(&sa_grid_bwd_k<decltype(tiles)::value, 8, DET>) : launch(&sa_grid_bwd_k<decltype(tiles)::value, 4, DET>); });
  if (rc) return rc;
  hipLaunchKernelGGL(sa_grid_dw_fold_k<F32>, dim3(kC * kC / 16), dim3(256), 0, stream, rois, partial, grad_w2, 0);
  FV2P_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace fv2p
using namespace fv2p;

extern "C" int fv2p_sa_grid_supported(int n, int m, int s, int c) {
  return (c == kC && (s == 16 || s == 32) && n >= 1 && m >= 1 && static_cast<size_t>(n) * kSaDp * 4 <= 114 * 1024) ? 1 : 0;   // backward: 45 KB of fragments / tiles (four waves) + the dP tile within 160 KB of LDS
}
extern "C" int fv2p_sa_grid_supported_h(int n, int m, int s, int c) {
  return (c == kC && (s == 16 || s == 32) && n >= 1 && m >= 1) ? 1 : 0;   // no dP tile in LDS: no limit on n
}

extern "C" int fv2p_sa_grid_fwd(const float* per_point, const float* per_centre, const int* idx, const float* w2, int rois, int n, int m,
                                int s, int c, float* out, unsigned char* arg, fv2p_stream_t stream) {
  FV2P_REQUIRE(shapes_ok(rois, n, m, s, c), FV2P_EINVAL, "sa_grid: needs 64 channels and 16 or 32 samples per centre");
  if (int rc = none_null("sa_grid_fwd", {per_point, per_centre, idx, w2, out})) return rc;
  with_tiles(s, [&](auto tiles) { launch_fwd<F32, decltype(tiles)::value, true>(per_point, per_centre, idx, w2, rois, n, m, out, arg, static_cast<hipStream_t>(stream)); });
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" int fv2p_sa_grid_fwd_h(const void* per_point, const void* per_centre, const int* idx, const void* w2, int wd, int rois, int n, int m,
                                  int s, int c, void* out, unsigned char* arg, int dtype, fv2p_stream_t stream) {
  if (int rc = dtypes_ok("sa_grid_fwd_h", dtype, wd)) return rc;
  FV2P_REQUIRE(shapes_ok(rois, n, m, s, c), FV2P_EINVAL, "sa_grid_fwd_h: needs 64 channels and 16 or 32 samples per centre");
  if (int rc = none_null("sa_grid_fwd_h", {per_point, per_centre, idx, w2, out})) return rc;
  if (int rc = all_aligned16("sa_grid_fwd_h", {per_point, per_centre, out, w2, arg})) return rc;
  with_instance16(dtype, s, wd, [&](auto f, auto tiles, auto w32) {
    launch_fwd<decltype(f), decltype(tiles)::value, decltype(w32)::value>(per_point, per_centre, idx, w2, rois, n, m, out, arg, static_cast<hipStream_t>(stream));
  });
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t fv2p_sa_grid_bwd_ws_bytes(int rois) {
  Sizer sz;
  sz.take<float>(static_cast<size_t>(rois > 0 ? rois : 1) * kC * kC);
  return sz.bytes();
}

extern "C" int fv2p_sa_grid_bwd(const float* per_point, const float* per_centre, const int* idx, const float* w2, const unsigned char* arg,
                                const float* grad_out, int rois, int n, int m, int s, int c, float* grad_point, float* grad_centre,
                                float* grad_w2, void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  FV2P_REQUIRE(shapes_ok(rois, n, m, s, c) && fv2p_sa_grid_supported(n, m, s, c), FV2P_EINVAL, "sa_grid_bwd: unsupported shape");
  if (int rc = none_null("sa_grid_bwd", {per_point, per_centre, idx, w2, arg, grad_out, grad_point, grad_centre, grad_w2})) return rc;
  FV2P_REQUIRE(ws && ws_bytes >= fv2p_sa_grid_bwd_ws_bytes(rois), FV2P_EWORKSPACE, "sa_grid_bwd: workspace too small");
  Carver cv(ws, ws_bytes);
  float* partial = cv.take<float>(static_cast<size_t>(rois) * kC * kC);
  return sa_grid_bwd_launch<false>(per_point, per_centre, idx, w2, arg, grad_out, rois, n, m, s, grad_point, grad_centre, grad_w2, partial, nullptr,
                                   static_cast<hipStream_t>(stream_));
}

extern "C" size_t fv2p_sa_grid_bwd_gather_ws_bytes(int rois, int m, int s) {
  return gather_ws_bytes(static_cast<size_t>(rois > 0 ? rois : 1), rois, m, s, sizeof(float));
}
extern "C" size_t fv2p_sa_grid_bwd_h_ws_bytes(int rois, int m, int s) {
  return gather_ws_bytes(static_cast<size_t>(rois > 0 ? rois : 1) * chunks_of(m), rois, m, s, sizeof(u16));
}

extern "C" int fv2p_sa_grid_bwd_gather(const float* per_point, const float* per_centre, const int* idx, const float* w2, const unsigned char* arg,
                                       const float* grad_out, int rois, int n, int m, int s, int c, float* grad_point, float* grad_centre,
                                       float* grad_w2, void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FV2P_REQUIRE(shapes_ok(rois, n, m, s, c) && fv2p_sa_grid_supported(n, m, s, c), FV2P_EINVAL, "sa_grid_bwd_gather: unsupported shape");
  if (int rc = none_null("sa_grid_bwd_gather", {per_point, per_centre, idx, w2, arg, grad_out, grad_point, grad_centre, grad_w2})) return rc;
  if (int rc = counts_fit("sa_grid_bwd_gather", rois, n, m, s)) return rc;
  FV2P_REQUIRE(ws && ws_bytes >= fv2p_sa_grid_bwd_gather_ws_bytes(rois, m, s), FV2P_EWORKSPACE, "sa_grid_bwd_gather: workspace too small");
  const int64_t entries = static_cast<int64_t>(rois) * m * s;
  const GatherWs w(Carver(ws, ws_bytes), static_cast<size_t>(rois), entries, sizeof(float));
  float* rows = static_cast<float*>(w.rows);
  if (int rc = sa_grid_bwd_launch<true>(per_point, per_centre, idx, w2, arg, grad_out, rois, n, m, s, grad_point, grad_centre, grad_w2, w.partial, rows,
                                        stream)) return rc;
  hipLaunchKernelGGL(sa_grid_entries_k, dim3(static_cast<unsigned>(ceil_div(entries, 256))), dim3(256), 0, stream, entries, n,
                     static_cast<int64_t>(m) * s, idx, w.dst);
  FV2P_HIP(hipMemsetAsync(grad_point, 0, static_cast<size_t>(rois) * n * kC * sizeof(float), stream));
  return fv2p_scatter_add(entries, kC, static_cast<int64_t>(rois) * n, w.dst, nullptr, nullptr, rows, 1, grad_point, w.sws, w.sws_bytes, stream);
}

extern "C" int fv2p_sa_grid_bwd_h(const void* per_point, const void* per_centre, const int* idx, const void* w2, int wd, const unsigned char* arg,
                                  const void* grad_out, int rois, int n, int m, int s, int c, void* grad_point, void* grad_centre, void* grad_w2,
                                  int dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = dtypes_ok("sa_grid_bwd_h", dtype, wd)) return rc;
  FV2P_REQUIRE(shapes_ok(rois, n, m, s, c), FV2P_EINVAL, "sa_grid_bwd_h: needs 64 channels and 16 or 32 samples per centre");
  if (int rc = none_null("sa_grid_bwd_h", {per_point, per_centre, idx, w2, arg, grad_out, grad_point, grad_centre, grad_w2})) return rc;
  if (int rc = all_aligned16("sa_grid_bwd_h", {per_point, per_centre, grad_out, w2, arg, grad_centre, grad_point, grad_w2})) return rc;
  if (int rc = counts_fit("sa_grid_bwd_h", rois, n, m, s)) return rc;
  FV2P_REQUIRE(ws && ws_bytes >= fv2p_sa_grid_bwd_h_ws_bytes(rois, m, s), FV2P_EWORKSPACE, "sa_grid_bwd_h: workspace too small");
  const int64_t entries = static_cast<int64_t>(rois) * m * s;
  const int parts = rois * chunks_of(m);
  const GatherWs w(Carver(ws, ws_bytes), static_cast<size_t>(parts), entries, sizeof(u16));
  u16* rows = static_cast<u16*>(w.rows);
  with_instance16(dtype, s, wd, [&](auto f, auto tiles, auto w32) {
    hipLaunchKernelGGL((sa_grid_bwd_h_k<decltype(f), decltype(tiles)::value, decltype(w32)::value>), dim3(static_cast<unsigned>(chunks_of(m)), rois), dim3(256), 0, stream, n, m,
                       static_cast<const u16*>(per_point), static_cast<const u16*>(per_centre), idx, w2, arg, static_cast<const u16*>(grad_out),
                       static_cast<u16*>(grad_centre), w.partial, rows);
  });
  with_format16(dtype, [&](auto f) {
    hipLaunchKernelGGL(sa_grid_dw_fold_k<decltype(f)>, dim3(kC * kC / 16), dim3(256), 0, stream, parts, w.partial, grad_w2, wd);
  });
  const int64_t per_roi = static_cast<int64_t>(m) * s;
  if (per_roi <= kPtMax && n <= kPtMaxN) {   // grad_point of a RoI inside one workgroup
    const int len = static_cast<int>(next_pow2(static_cast<uint64_t>(per_roi)));
    with_format16(dtype, [&](auto f) {
      hipLaunchKernelGGL(sa_grid_points_h_k<decltype(f)>, dim3(rois), dim3(512), 0, stream, n, static_cast<int>(per_roi), len, idx, rows,
                         static_cast<u16*>(grad_point));
    });
    FV2P_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL(sa_grid_entries_k, dim3(static_cast<unsigned>(ceil_div(entries, 256))), dim3(256), 0, stream, entries, n, per_roi, idx, w.dst);
  FV2P_LAUNCH_CHECK();
  return scatter_add_h(entries, kC, static_cast<int64_t>(rois) * n, w.dst, nullptr, nullptr, rows, 1, grad_point, dtype, w.sws, w.sws_bytes, stream);
}
