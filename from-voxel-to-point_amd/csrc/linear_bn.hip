// nn.Linear(bias=False) -> nn.BatchNorm1d [-> nn.ReLU] over point rows: the thirteen layers of the voxel-to-point decoder
// (fv2p_harness/fv2p_model.py: LateralBlock.net / .downsample, V2PDecoder.decode_block_out) and BEVGridPooling's compression, on fp32
// rows and - after .half(), .bfloat16() or under autocast - on float16 / bfloat16 rows.  One source, three storage formats (G32, MH, MB
// below, built on bn_fmt.hpp's F32 and Fmt16<T>).
//
//   x [n][cin], w [cout][cin] (the module's weight as it stands), z = x * w^T [n][cout]
//   forward (training)  z, per-channel sum z / sum z^2 from the GEMM's epilogue -> mean, invstd, running statistics -> y
//   forward (eval)      y = relu?((z - mean) * invstd * gamma + beta) in the GEMM's epilogue, one launch
//   backward            dz = dy * [y > 0] (mask recomputed from z), dgamma, dbeta, du = gamma * invstd * (dz - c1 - xhat * c2);
//                       dx = du * w;  dw = du^T * x
//
// Arithmetic contract of the 16-bit formats.  T is float16 or bfloat16 (dt).  x [n][cin] in T; w [cout][cin] in T or fp32 (wd); an fp32
// weight is rounded ONCE to T on its way into LDS (the bits of w.to(T); no 16-bit copy of the weight in memory); gamma, beta, the
// running statistics and dgamma / dbeta are fp32 or T (pd); mean and invstd are fp32.
//   1. pre-activation   acc = sum_k x * w on v_mfma_f32_16x16x32_{f16,bf16}: a product of two T values is exact, the accumulators are
//                       fp32 in a fixed order.  z = round_T(acc) is stored [n][cout] in T and IS the op's pre-activation everywhere:
//                       everything downstream reads the stored 16-bit z, widened (torch's bn(linear(x)) on 16-bit rows), so the
//                       forward pass and the ReLU mask the backward pass recomputes agree by construction.
//   2. training mode    per-channel sum z / sum z^2 of the ROUNDED z from the GEMM's epilogue, fp64 partials per row tile, folded in
//                       a fixed order of the tiles by a later launch; mean / invstd fp32; running statistics and num_batches_tracked through
//                       bn_fwd_channel (bn_fold.hpp) in the parameters' format (momentum, momentum=None, unbiased variance); then
//                       y = round_T(relu?((z - mean) * invstd * gamma + beta)) in fp32.
//   3. eval mode        one launch; z = round_T(acc) is stored only when a buffer is passed; y from the widened z with the caller's
//                       fp32 mean / invstd.
//   4. backward         the ReLU mask from z with the forward's expression; dgamma, dbeta, c1, c2 from fp64 sums in a fixed order;
//                       du = gamma * invstd * (dz - c1 - xhat * c2) in fp32, rounded ONCE to T: the staging buffer and the MFMA
//                       operand.  dx = du * w: fp32 accumulators, one rounding to T.  dw = du^T * x over a fixed split of the rows,
//                       folded in split order and rounded once (to_odd, then T::round) into a T weight, or stored as fp32 for an fp32
//                       master weight.  dgamma / dbeta in the parameters' format.
// fp32 rows are the same sentences with round_T the identity: the stored value is the accumulator.
//
// One tile GEMM serves the four products (lbn_gemm_k): a workgroup of four waves owns 128 output rows x 64 output columns, wave v the
// rows 32 v .. 32 v + 31 as 2 x 4 tiles of 16 x 16: D[i = 4 * lk + r][j = li] comes back in register r of lane 16 * lk + li.  Both
// operands stream through LDS in K chunks; the next chunk's global loads are issued before this chunk's MFMAs.  Ragged extents are
// zero-filled on load (branch-free guarded loads, as head1x1.hip) and never stored; a width that is no multiple of the format's vector,
// or a base that is not 16-byte aligned, takes the element-wise load path.  What a format brings of its own (Tile, kKC, kFlush, frag, mfma):
//   G32     v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate; there is no xf32 on gfx950): A[i = li][k = lk], B[k = lk][j = li].  K chunks
//           of 16, stored K-major ([k][row], the row stride 16 banks past a multiple of 64 so that the four K rows a fragment read touches
//           fall on different banks).  An operand is either K-contiguous in memory (x and w forward, du in backward data: 16-byte loads
//           along K, transposed on the way into LDS) or row-contiguous (w in backward data, du and x in backward weights: copied as it
//           lies).
//   MH, MB  v_mfma_f32_16x16x32_{f16,bf16}: lane l holds A[l & 15][8 (l >> 4) + j] and B[8 (l >> 4) + j][l & 15].  K chunks of 64 as
//           [row][k] images (row stride 72 elements: 16-byte aligned; the 16-byte K groups of a row are permuted by (row / 8) % 8 so that
//           the transposing stores of the weight-gradient pass spread over the banks), read as one 16-byte fragment per lane and MFMA.
//           Forward: x and w are K-contiguous, 16-byte global loads, 16-byte LDS stores.  Backward data: w^T is materialised in T in the
//           workspace per call (lbn_wt_k: <= 1 MB; it also rounds an fp32 master weight), so the product has the forward's form.
//           Backward weights: K = rows, neither operand K-contiguous: 16-byte loads along the channels of two rows, and the pair of rows
//           goes into the [channel][row] image as one 32-bit LDS store per channel.
//
// No float atomics and no workgroup waits for another: the statistics leave the forward GEMM as one partial row per row tile, the weight
// gradient as one fp64 partial tile per row chunk, and a later launch on the same stream folds them in a fixed order: bit-identical
// results from run to run.  The weight gradient accumulates 128 rows (kFlush chunks) in the fp32 MFMA accumulators, then adds them into
// fp64 sums held in registers, so no fp32 chain is longer than 128 terms whatever n is.
#include <algorithm>

#include "common.hpp"
#include "bn_fold.hpp"

namespace fv2p {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
using f16x8 = _Float16 __attribute__((ext_vector_type(8)));
using bf16x8 = __bf16 __attribute__((ext_vector_type(8)));

constexpr int kBM = 128;          // output rows per workgroup (the A operand's side): 4 waves x 32
constexpr int kBN = 64;           // output columns per workgroup (the B operand's side)
constexpr int kSplitRows = 128;   // backward weights: rows (kFlush chunks of kKC) between two additions into the fp64 sums
constexpr int kMaxCin = 1024, kMaxCout = 512;
constexpr int kSumUnits = 32, kSumLanes = 8;    // backward BatchNorm sums: 32 units of V columns x 8 row lanes at a time
constexpr int kRedRows = 64;      // backward BatchNorm sums: at least this many rows per workgroup
constexpr int kRedBlocks = 1024;  // ... and at most this many workgroups
constexpr int64_t kWgBytes = 16ll << 20;   // backward weights: at most this many bytes of fp64 partial tiles

enum Mode { kFwdTrain, kFwdEval, kData, kWeights };

// Guarded loads without a branch (head1x1.hip): an address that is always readable and the value 0 outside.
__device__ __forceinline__ float ld_or0(const float* p, bool ok, const float* safe) {
  const float v = *(ok ? p : safe);
  return ok ? v : 0.f;
}
__device__ __forceinline__ float4 ld4_or0(const float* p, bool ok, const float* safe) {
  const float4 v = *reinterpret_cast<const float4*>(ok ? p : safe);
  return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ uint4 ld8_or0(const u16* p, bool ok, const void* safe) {
  const uint4 v = *reinterpret_cast<const uint4*>(ok ? static_cast<const void*>(p) : safe);
  return ok ? v : make_uint4(0u, 0u, 0u, 0u);
}
__device__ __forceinline__ unsigned ld1_or0(const u16* p, bool ok, const void* safe) {
  const u16 v = *(ok ? p : static_cast<const u16*>(safe));
  return ok ? static_cast<unsigned>(v) : 0u;
}
template <class T>
__device__ __forceinline__ unsigned ld1f_or0(const float* p, bool ok, const void* safe) {   // an fp32 weight: rounded once to T
  const float v = *(ok ? p : static_cast<const float*>(safe));
  return ok ? static_cast<unsigned>(T::round(v)) : 0u;
}
__device__ __forceinline__ unsigned half_of(const uint4& v, int e) {
  const unsigned w = e < 2 ? v.x : e < 4 ? v.y : e < 6 ? v.z : v.w;
  return (w >> (16 * (e & 1))) & 0xffffu;
}

// ---- the formats: F32 / Fmt16<T> of bn_fmt.hpp plus what the tile GEMM and the folds need of each.  Tile<ROWS, KCONT, VEC, SRC32> is a
// thread's share of a ROWS x kKC operand tile: element (row, k) of the operand is p[row * ld + k] (KCONT) or p[k * ld + row]; load()
// takes it from memory (rows r0 .. rlim, K k0 .. klim, zeros outside), store() puts it into the operand's LDS region of kLds<ROWS>
// elements; frag() reads a lane's A or B fragment of MFMA step ks (of kSteps per chunk) from such a region, mfma() is the instruction. ------
struct G32 : F32 {
  static constexpr bool k16 = false;   // backward data reads w row-contiguous in place; the weight is always fp32
  static constexpr int kKC = 16;       // K per LDS chunk
  static constexpr int kFlush = 8;     // backward weights: K chunks between two additions into the fp64 sums
  static constexpr int kFoldCols = 32, kFoldLanes = 8;   // the fold kernels: 32 columns x 8 interleaved row lanes per workgroup
  static constexpr int kSumVec = 1, kSumUnroll = 4;   // backward BatchNorm sums: one column per thread, four rows in flight
  template <int ROWS>
  static constexpr int kLds = kKC * (ROWS + 16);   // K-major: ROWS + 16 floats per K row

  // NV groups of 4 floats, along K (KCONT) or along the rows
  template <int ROWS, bool KCONT, bool VEC, bool SRC32>
  struct Tile {
    static constexpr int NV = ROWS * kKC / 4 / 256;
    static constexpr int LD = ROWS + 16;
    float4 r[NV];
    __device__ __forceinline__ void load(const void* __restrict__ base, long long ld, long long r0, long long rlim, long long k0, long long klim) {
      const float* __restrict__ p = static_cast<const float*>(base);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int f = threadIdx.x + 256 * i;
        if constexpr (KCONT) {
          const long long gr = r0 + (f >> 2), gk = k0 + 4 * (f & 3);
          const float* q = p + gr * ld + gk;
          const bool ok = gr < rlim;
          if constexpr (VEC) r[i] = ld4_or0(q, ok && gk < klim, p);   // ld % 4 == 0: a group is inside the row or outside
          else r[i] = make_float4(ld_or0(q, ok && gk < klim, p), ld_or0(q + 1, ok && gk + 1 < klim, p), ld_or0(q + 2, ok && gk + 2 < klim, p),
                                  ld_or0(q + 3, ok && gk + 3 < klim, p));
        } else {
          const long long gk = k0 + f / (ROWS / 4), gr = r0 + 4 * (f % (ROWS / 4));
          const float* q = p + gk * ld + gr;
          const bool ok = gk < klim;
          if constexpr (VEC) r[i] = ld4_or0(q, ok && gr < rlim, p);
          else r[i] = make_float4(ld_or0(q, ok && gr < rlim, p), ld_or0(q + 1, ok && gr + 1 < rlim, p), ld_or0(q + 2, ok && gr + 2 < rlim, p),
                                  ld_or0(q + 3, ok && gr + 3 < rlim, p));
        }
      }
    }
    __device__ __forceinline__ void store(float* s) const {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int f = threadIdx.x + 256 * i;
        if constexpr (KCONT) {
          float* q = s + 4 * (f & 3) * LD + (f >> 2);
          q[0] = r[i].x; q[LD] = r[i].y; q[2 * LD] = r[i].z; q[3 * LD] = r[i].w;
        } else {
          *reinterpret_cast<float4*>(s + (f / (ROWS / 4)) * LD + 4 * (f % (ROWS / 4))) = r[i];
        }
      }
    }
  };

  // one MFMA step is K = 4: lane (lk, li) reads element (row, 4 ks + lk) of an operand
  static constexpr int kSteps = kKC / 4;
  using Frag = float;
  template <int ROWS>
  static __device__ __forceinline__ float frag(const float* s, int row, int ks, int lk) { return s[(4 * ks + lk) * (ROWS + 16) + row]; }
  static __device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
};

struct CvtH : H16 {
  static __device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};
struct CvtB : B16 {
  static __device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};

template <class T>   // T: widen, round and mfma
struct G16 : Fmt16<T> {
  static constexpr bool k16 = true;    // backward data reads w^T from the workspace (lbn_wt_k); the weight is T or fp32
  static constexpr int kKC = 64;       // K per LDS chunk: two MFMA steps of 32
  static constexpr int kFlush = 2;
  static constexpr int kFoldCols = 8, kFoldLanes = 32;   // the fold kernels: 8 columns x 32 interleaved row lanes per workgroup
  static constexpr int kSumVec = 8, kSumUnroll = 2;   // ... one 16-byte unit per thread where the rows allow it, two rows in flight
  static constexpr int kLd = kKC + 8;  // elements per image row
  template <int ROWS>
  static constexpr int kLds = ROWS * kLd;

  // element offset of (row, k) in a [ROWS][kLd] image: the 16-byte K groups of a row are permuted by (row / 8) % 8
  static __device__ __forceinline__ int img(int row, int k) { return row * kLd + ((((k >> 3) ^ (row >> 3)) & 7) << 3) + (k & 7); }

  // NV units of 8 elements, along K (KCONT) or along the rows.  SRC32: the operand is fp32 in memory (KCONT only).  Units along the
  // rows come in pairs (2 j, 2 j + 1) = rows k, k + 1 of the same 8 channels.
  template <int ROWS, bool KCONT, bool VEC, bool SRC32>
  struct Tile {
    static constexpr int NV = ROWS * kKC / 8 / 256;
    static constexpr int G = ROWS / 8;
    uint4 r[NV];
    __device__ __forceinline__ void load(const void* __restrict__ base, long long ld, long long r0, long long rlim, long long k0, long long klim) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        if constexpr (KCONT) {
          const int f = threadIdx.x + 256 * i;
          const long long gr = r0 + (f >> 3), gk = k0 + 8 * (f & 7);
          const bool ok = gr < rlim;
          unsigned e[8];
          if constexpr (SRC32) {
            const float* q = static_cast<const float*>(base) + gr * ld + gk;
            if constexpr (VEC) {   // ld % 8 == 0: a group is inside the row or outside
              const bool in = ok && gk < klim;
              const float4 lo = *reinterpret_cast<const float4*>(in ? static_cast<const void*>(q) : base);
              const float4 hi = *reinterpret_cast<const float4*>(in ? static_cast<const void*>(q + 4) : base);
              const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
              for (int j = 0; j < 8; ++j) e[j] = in ? static_cast<unsigned>(T::round(v[j])) : 0u;
            } else {
#pragma unroll
              for (int j = 0; j < 8; ++j) e[j] = ld1f_or0<T>(q + j, ok && gk + j < klim, base);
            }
            r[i] = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
          } else {
            const u16* q = static_cast<const u16*>(base) + gr * ld + gk;
            if constexpr (VEC) r[i] = ld8_or0(q, ok && gk < klim, base);
            else {
#pragma unroll
              for (int j = 0; j < 8; ++j) e[j] = ld1_or0(q + j, ok && gk + j < klim, base);
              r[i] = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
            }
          }
        } else {
          const int f = threadIdx.x + 256 * (i >> 1);
          const long long gk = k0 + 2 * (f / G) + (i & 1), gr = r0 + 8 * (f % G);
          const u16* q = static_cast<const u16*>(base) + gk * ld + gr;
          const bool ok = gk < klim;
          if constexpr (VEC) r[i] = ld8_or0(q, ok && gr < rlim, base);   // ld % 8 == 0 and rlim == ld
          else {
            unsigned e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = ld1_or0(q + j, ok && gr + j < rlim, base);
            r[i] = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
          }
        }
      }
    }
    __device__ __forceinline__ void store(u16* s) const {
      if constexpr (KCONT) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const int f = threadIdx.x + 256 * i;
          *reinterpret_cast<uint4*>(s + img(f >> 3, 8 * (f & 7))) = r[i];
        }
      } else {
#pragma unroll
        for (int p = 0; p < NV / 2; ++p) {
          const int f = threadIdx.x + 256 * p;
          const int k = 2 * (f / G), row = 8 * (f % G);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            *reinterpret_cast<unsigned*>(s + img(row + j, k)) = half_of(r[2 * p], j) | (half_of(r[2 * p + 1], j) << 16);
        }
      }
    }
  };

  // one MFMA step is K = 32: lane (lk, li) reads the 8 elements (row, 32 ks + 8 lk ..) of an operand as one 16-byte fragment
  static constexpr int kSteps = kKC / 32;
  using Frag = uint4;
  template <int ROWS>
  static __device__ __forceinline__ uint4 frag(const u16* s, int row, int ks, int lk) { return *reinterpret_cast<const uint4*>(s + img(row, 32 * ks + 8 * lk)); }
  static __device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) { return T::mfma(a, b, c); }
};
using MH = G16<CvtH>;
using MB = G16<CvtB>;
static_assert(G32::kFlush * G32::kKC == kSplitRows && MH::kFlush * MH::kKC == kSplitRows, "one geometry of the weight-gradient splits");

template <class F>
struct Gemm {
  const void* a;    // M side operand
  const void* b;    // N side operand (fp32 where the kernel's B32 says so)
  long long lda, ldb;
  long long m, n, k;      // output rows, output columns, length of the sum
  typename F::elem* out;  // [m][n]: z (may be null in eval mode) or dx
  double* part;           // kFwdTrain: [row tiles][2][n] sums; kWeights: [splits][m][n] partial tiles
  long long chunk;        // kWeights: K per split (a multiple of kSplitRows)
  const float* mean; const float* invstd; const void* gamma; const void* beta; int pd;   // kFwdEval
  int relu;
  typename F::elem* y;
};

template <class F, int MODE, bool VEC, bool B32>
__global__ __launch_bounds__(256) void lbn_gemm_k(const Gemm<F> g) {
  constexpr bool A_KCONT = MODE != kWeights, B_KCONT = MODE == kFwdTrain || MODE == kFwdEval || (MODE == kData && F::k16);
  __shared__ __attribute__((aligned(16))) typename F::elem as[F::template kLds<kBM>];
  __shared__ __attribute__((aligned(16))) typename F::elem bs[F::template kLds<kBN>];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const long long m0 = static_cast<long long>(blockIdx.x) * kBM, n0 = static_cast<long long>(blockIdx.y) * kBN;
  const long long k_begin = MODE == kWeights ? static_cast<long long>(blockIdx.z) * g.chunk : 0;
  const long long k_end = MODE == kWeights ? min(k_begin + g.chunk, g.k) : g.k;
  f32x4 acc[2][4];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) acc[mi][nj] = f32x4{0.f, 0.f, 0.f, 0.f};
  double dacc[MODE == kWeights ? 32 : 1];
  if constexpr (MODE == kWeights) {
#pragma unroll
    for (int i = 0; i < 32; ++i) dacc[i] = 0.0;
  }
  auto flush = [&]() {
    if constexpr (MODE == kWeights) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nj = 0; nj < 4; ++nj)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            dacc[(mi * 4 + nj) * 4 + r] += static_cast<double>(acc[mi][nj][r]);
            acc[mi][nj][r] = 0.f;
          }
    }
  };
  typename F::template Tile<kBM, A_KCONT, VEC, false> ta;
  typename F::template Tile<kBN, B_KCONT, VEC, B32> tb;
  ta.load(g.a, g.lda, m0, g.m, k_begin, k_end);
  tb.load(g.b, g.ldb, n0, g.n, k_begin, k_end);
  int since = 0;
  for (long long k0 = k_begin; k0 < k_end; k0 += F::kKC) {
    __syncthreads();
    ta.store(as);
    tb.store(bs);
    __syncthreads();
    // the next chunk's loads fly during this one's MFMAs (past k_end they are guarded away)
    ta.load(g.a, g.lda, m0, g.m, k0 + F::kKC, k_end);
    tb.load(g.b, g.ldb, n0, g.n, k0 + F::kKC, k_end);
#pragma unroll
    for (int ks = 0; ks < F::kSteps; ++ks) {
      typename F::Frag av[2], bv[4];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) av[mi] = F::template frag<kBM>(as, wave * 32 + mi * 16 + li, ks, lk);
#pragma unroll
      for (int nj = 0; nj < 4; ++nj) bv[nj] = F::template frag<kBN>(bs, nj * 16 + li, ks, lk);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nj = 0; nj < 4; ++nj) acc[mi][nj] = F::mfma(av[mi], bv[nj], acc[mi][nj]);
    }
    if constexpr (MODE == kWeights) {
      if (++since == F::kFlush) { flush(); since = 0; }
    }
  }
  // D row 4 * lk + r of tile (mi, nj) is output row m0 + 32 * wave + 16 * mi + 4 * lk + r, column n0 + 16 * nj + li
  const long long row_base = m0 + wave * 32 + 4 * lk;
  if constexpr (MODE == kWeights) {
    flush();
    double* part = g.part + static_cast<long long>(blockIdx.z) * g.m * g.n;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int nj = 0; nj < 4; ++nj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long row = row_base + mi * 16 + r, col = n0 + nj * 16 + li;
          if (row < g.m && col < g.n) part[row * g.n + col] = dacc[(mi * 4 + nj) * 4 + r];
        }
  } else if constexpr (MODE == kFwdEval) {
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const long long col = n0 + nj * 16 + li;
      if (col >= g.n) continue;
      const int e = static_cast<int>(col);
      const float mu = g.mean[e], is = g.invstd[e], ga = F::par_load(g.gamma, e, g.pd, 1.f), be = F::par_load(g.beta, e, g.pd, 0.f);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long row = row_base + mi * 16 + r;
          if (row >= g.m) continue;
          const typename F::elem zb = F::narrow(acc[mi][nj][r]);
          const float z = F::widen(zb);
          const float t = (z - mu) * is * ga + be;
          if (g.out) g.out[row * g.n + col] = zb;
          g.y[row * g.n + col] = F::narrow((g.relu && t <= 0.f) ? 0.f : t);   // NaN passes through, like torch.relu
        }
    }
  } else {
    // z (or dx) in the storage format; the forward's sums below are those of the stored values
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int nj = 0; nj < 4; ++nj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long row = row_base + mi * 16 + r, col = n0 + nj * 16 + li;
          const typename F::elem zb = F::narrow(acc[mi][nj][r]);
          if (row < g.m && col < g.n) g.out[row * g.n + col] = zb;
          if constexpr (MODE == kFwdTrain) acc[mi][nj][r] = F::widen(zb);
        }
  }
  if constexpr (MODE == kFwdTrain) {
    // sum z and sum z^2 of this workgroup's 128 rows, per column, in fp64 (rows past m are zero rows): the lane's 8 rows, the
    // 4 lanes of a column (lk), then the 4 waves in wave order
    __shared__ double red[4][kBN][2];
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      double s = 0.0, q = 0.0;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double v = static_cast<double>(acc[mi][nj][r]);
          s += v;
          q += v * v;
        }
      s += __shfl_xor(s, 16, 64); q += __shfl_xor(q, 16, 64);
      s += __shfl_xor(s, 32, 64); q += __shfl_xor(q, 32, 64);
      if (lk == 0) { red[wave][nj * 16 + li][0] = s; red[wave][nj * 16 + li][1] = q; }
    }
    __syncthreads();
    if (tid < kBN && n0 + tid < g.n) {
      const double s = ((red[0][tid][0] + red[1][tid][0]) + red[2][tid][0]) + red[3][tid][0];
      const double q = ((red[0][tid][1] + red[1][tid][1]) + red[2][tid][1]) + red[3][tid][1];
      g.part[(static_cast<long long>(blockIdx.x) * 2 + 0) * g.n + n0 + tid] = s;
      g.part[(static_cast<long long>(blockIdx.x) * 2 + 1) * g.n + n0 + tid] = q;
    }
  }
}

// w [cout][cin] (T, or fp32 rounded once) -> wt [cin][cout] in T: the B operand of the 16-bit backward data product
template <class F, bool W32>
__global__ __launch_bounds__(256) void lbn_wt_k(const void* __restrict__ w, int cout, int cin, u16* __restrict__ wt) {
  __shared__ u16 tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int co = co0 + ty + 8 * j, ci = ci0 + tx;
    u16 v = 0;
    if (co < cout && ci < cin) {
      const long long e = static_cast<long long>(co) * cin + ci;
      if constexpr (W32) v = F::narrow(static_cast<const float*>(w)[e]);
      else v = static_cast<const u16*>(w)[e];
    }
    tile[ty + 8 * j][tx] = v;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ci = ci0 + ty + 8 * j, co = co0 + tx;
    if (ci < cin && co < cout) wt[static_cast<long long>(ci) * cout + co] = tile[tx][ty + 8 * j];
  }
}

// ---- fold of the [rows][2][c] partial sums: a workgroup takes F::kFoldCols columns, F::kFoldLanes lanes per column walk interleaved
// rows, then an ordered LDS fold (the geometry is the format's: it fixes the order of the additions, and so the bits).  Forward: mean,
// invstd and the running statistics in the parameters' format (bn_fwd_channel: the arithmetic of every BatchNorm of the library); every
// column reads *num_batches_tracked (momentum=None) and nobody in this launch writes it: the apply launch that follows does.
// Backward: dbeta, dgamma (the parameters' format) and the two means of the input gradient (fp32). -----------------------------------
template <class F, bool BWD>
__global__ __launch_bounds__(256) void lbn_fold_k(const double* __restrict__ part, int rows, long long n, int c, BnFwdFin ff, void* running_mean,
                                                  void* running_var, void* dgamma, void* dbeta, float* coef, int batch_stats, int pd) {
  constexpr int kFoldCols = F::kFoldCols, kFoldLanes = F::kFoldLanes;
  __shared__ double red[2][kFoldLanes][kFoldCols];
  const int tid = threadIdx.x, cl = tid % kFoldCols, rl = tid / kFoldCols, col = blockIdx.x * kFoldCols + cl;
  double a = 0.0, b = 0.0;
  if (col < c) {
#pragma unroll 4
    for (int q = rl; q < rows; q += kFoldLanes) {
      a += part[(static_cast<long long>(q) * 2 + 0) * c + col];
      b += part[(static_cast<long long>(q) * 2 + 1) * c + col];
    }
  }
  red[0][rl][cl] = a; red[1][rl][cl] = b;
  __syncthreads();
  if (rl != 0 || col >= c) return;
  a = 0.0; b = 0.0;
  for (int q = 0; q < kFoldLanes; ++q) { a += red[0][q][cl]; b += red[1][q][cl]; }
  if constexpr (!BWD) {
    float mu, is;
    bn_fwd_channel<F>(a, b, n, ff, running_mean, running_var, pd, col, true, &mu, &is);
  } else {
    const double nn = static_cast<double>(n);
    if (dbeta) F::par_store(dbeta, col, pd, a);
    if (dgamma) F::par_store(dgamma, col, pd, b);
    coef[col] = batch_stats ? static_cast<float>(a / nn) : 0.f;
    coef[c + col] = batch_stats ? static_cast<float>(b / nn) : 0.f;
  }
}

// per-column constants of the element-wise passes, staged in LDS once per workgroup
struct Cols {
  float mean[kMaxCout], is[kMaxCout], gamma[kMaxCout], beta[kMaxCout];
};
template <class F>
__device__ __forceinline__ void cols_load(Cols& s, int c, const float* mean, const float* invstd, const void* gamma, const void* beta, int pd) {
  for (int e = threadIdx.x; e < c; e += 256) {
    s.mean[e] = mean[e];
    s.is[e] = invstd[e];
    s.gamma[e] = F::par_load(gamma, e, pd, 1.f);
    s.beta[e] = F::par_load(beta, e, pd, 0.f);
  }
}

// y = relu?((z - mean) * invstd * gamma + beta), rounded once; units of V elements (V = F::kVec: c % V == 0).  The launch comes after
// the fold, so its first thread is the one that advances num_batches_tracked (null: not tracked).
template <class F, int V>
__global__ __launch_bounds__(256) void lbn_apply_k(const typename F::elem* __restrict__ z, long long units, int c, const float* __restrict__ mean,
                                                   const float* __restrict__ invstd, const void* __restrict__ gamma,
                                                   const void* __restrict__ beta, int pd, int relu, typename F::elem* __restrict__ y,
                                                   long long* nbt) {
  __shared__ Cols s;
  cols_load<F>(s, c, mean, invstd, gamma, beta, pd);
  __syncthreads();
  if (nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;
  const int cv = c / V;
  for (long long u = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; u < units; u += static_cast<long long>(gridDim.x) * 256) {
    const int col = static_cast<int>(u % cv) * V;
    typename F::template Unit<V> zv, o;
    zv.load(z + u * V);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float t = (zv.v[i] - s.mean[col + i]) * s.is[col + i] * s.gamma[col + i] + s.beta[col + i];
      o.v[i] = (relu && t <= 0.f) ? 0.f : t;
    }
    o.store(y + u * V);
  }
}

// backward BatchNorm sums: workgroup b takes rows [b * rpb, (b + 1) * rpb) and leaves sum dz, sum dz * xhat per column in
// part[b][2][c].  32 units of V columns x 8 row lanes at a time (V = 8: c % 8 == 0, one 16-byte access per tensor and row; fp32 rows
// run V = 1); a thread sums its rows in row order, the row lanes are folded in lane order through LDS.
template <class F, int V>
__global__ __launch_bounds__(256) void lbn_bwd_sums_k(const typename F::elem* __restrict__ z, const typename F::elem* __restrict__ dy, long long n,
                                                      int c, long long rpb, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                      const void* __restrict__ gamma, const void* __restrict__ beta, int pd, int relu,
                                                      double* __restrict__ part) {
  __shared__ double red[2][kSumLanes][kSumUnits * V];
  const int tid = threadIdx.x, cl = tid % kSumUnits, rl = tid / kSumUnits;
  const long long r0 = static_cast<long long>(blockIdx.x) * rpb, r1 = min(r0 + rpb, n);
  for (int c0 = 0; c0 < c; c0 += kSumUnits * V) {
    const int col = c0 + cl * V;   // (c % V == 0: a unit is inside the row or outside)
    double a[V], b[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { a[i] = 0.0; b[i] = 0.0; }
    if (col < c) {
      float mu[V], is[V], ga[V], be[V];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        mu[i] = mean[col + i]; is[i] = invstd[col + i];
        ga[i] = F::par_load(gamma, col + i, pd, 1.f); be[i] = F::par_load(beta, col + i, pd, 0.f);
      }
#pragma unroll F::kSumUnroll
      for (long long r = r0 + rl, at = r * c + col; r < r1; r += kSumLanes, at += static_cast<long long>(kSumLanes) * c) {
        typename F::template Unit<V> zv, gv;
        zv.load(z + at);
        gv.load(dy + at);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const float xhat = (zv.v[i] - mu[i]) * is[i];
          const float t = xhat * ga[i] + be[i];
          const float dz = (relu && !(t > 0.f)) ? 0.f : gv.v[i];
          a[i] += dz;
          b[i] += static_cast<double>(dz) * xhat;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < V; ++i) { red[0][rl][cl * V + i] = a[i]; red[1][rl][cl * V + i] = b[i]; }
    __syncthreads();
    if (tid < kSumUnits * V && c0 + tid < c) {   // (at most 256 columns at a time: one per thread)
      double sa = 0.0, sb = 0.0;
      for (int q = 0; q < kSumLanes; ++q) { sa += red[0][q][tid]; sb += red[1][q][tid]; }
      part[(static_cast<long long>(blockIdx.x) * 2 + 0) * c + c0 + tid] = sa;
      part[(static_cast<long long>(blockIdx.x) * 2 + 1) * c + c0 + tid] = sb;
    }
  }
}

// du = gamma * invstd * (dz - c1 - xhat * c2), rounded once: the gradient of the pre-activation z (coef = [c1][c2], zeros for a frozen
// BatchNorm)
template <class F, int V>
__global__ __launch_bounds__(256) void lbn_du_k(const typename F::elem* __restrict__ z, const typename F::elem* __restrict__ dy, long long units,
                                                int c, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                const void* __restrict__ gamma, const void* __restrict__ beta, int pd, int relu,
                                                const float* __restrict__ coef, typename F::elem* __restrict__ du) {
  __shared__ Cols s;
  __shared__ float c1[kMaxCout], c2[kMaxCout];
  cols_load<F>(s, c, mean, invstd, gamma, beta, pd);
  for (int e = threadIdx.x; e < c; e += 256) { c1[e] = coef[e]; c2[e] = coef[c + e]; }
  __syncthreads();
  const int cv = c / V;
  for (long long u = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; u < units; u += static_cast<long long>(gridDim.x) * 256) {
    const int col = static_cast<int>(u % cv) * V;
    typename F::template Unit<V> zv, gv, o;
    zv.load(z + u * V);
    gv.load(dy + u * V);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float is = s.is[col + i], ga = s.gamma[col + i];
      const float xhat = (zv.v[i] - s.mean[col + i]) * is;
      const float t = xhat * ga + s.beta[col + i];
      const float dz = (relu && !(t > 0.f)) ? 0.f : gv.v[i];
      o.v[i] = ga * is * (dz - c1[col + i] - xhat * c2[col + i]);
    }
    o.store(du + u * V);
  }
}

// dw[e] = the fp64 partials of element e summed in split order, one rounding at the store (W32: into an fp32 weight gradient)
template <class F, bool W32>
__global__ __launch_bounds__(256) void lbn_dw_fold_k(const double* __restrict__ part, int splits, long long elems, void* __restrict__ dw) {
  const long long e = blockIdx.x * 256ll + threadIdx.x;
  if (e >= elems) return;
  double acc = 0.0;
  for (int s0 = 0; s0 < splits; s0 += 8) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = s0 + i < splits ? part[(s0 + i) * elems + e] : 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc += v[i];
  }
  F::par_store(dw, static_cast<int>(e), W32 ? 0 : 1, acc);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct Geom {
  int64_t n;
  int cin, cout;
  int64_t row_tiles;    // forward GEMM: partial rows of the statistics
  int64_t red_blocks, red_rpb;   // backward BatchNorm sums
  int64_t split_bound;  // backward weights: what the workspace is sized for (never decreases with n)
  int64_t chunk;
  int splits;
};

bool shape_ok(int64_t n, int cin, int cout) { return n >= 1 && n <= INT32_MAX && cin >= 1 && cin <= kMaxCin && cout >= 1 && cout <= kMaxCout; }
bool dt_ok(int dt) { return dt == FV2P_DT_F16 || dt == FV2P_DT_BF16; }
bool formats_ok(int dt, int wd, int pd) { return dt_ok(dt) && (wd == 0 || wd == dt) && (pd == 0 || pd == dt); }

Geom geom(int64_t n, int cin, int cout) {
  Geom g;
  g.n = n; g.cin = cin; g.cout = cout;
  g.row_tiles = ceil_div(n, kBM);
  g.red_rpb = std::max<int64_t>(kRedRows, ceil_div(n, kRedBlocks));
  g.red_blocks = ceil_div(n, g.red_rpb);
  // row chunks of the weight gradient: about four workgroups per CU, no more than kWgBytes of partial tiles, whole flush periods
  const int64_t tiles = ceil_div(cout, kBM) * ceil_div(cin, kBN);
  const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(1024 / tiles, kWgBytes / (static_cast<int64_t>(cout) * cin * 8)));
  g.split_bound = std::min<int64_t>(ceil_div(n, kSplitRows), cap);
  g.chunk = ceil_div(ceil_div(n, g.split_bound), kSplitRows) * kSplitRows;
  g.splits = static_cast<int>(ceil_div(n, g.chunk));
  return g;
}

struct Ws {
  double* stats;   // [max(row_tiles, red_blocks)][2][cout]
  float* coef;     // [2][cout]
  double* wpart;   // [splits][cout][cin]
  u16* wt;         // [cin][cout], the 16-bit formats only
};
template <typename C>
Ws carve(C& cv, const Geom& g, bool h) {
  Ws w;
  w.stats = cv.template take<double>(static_cast<size_t>(std::max(g.row_tiles, g.red_blocks)) * 2 * g.cout);
  w.coef = cv.template take<float>(2 * static_cast<size_t>(g.cout));
  w.wpart = cv.template take<double>(static_cast<size_t>(g.split_bound) * g.cout * g.cin);
  w.wt = h ? cv.template take<u16>(static_cast<size_t>(g.cout) * g.cin) : nullptr;
  return w;
}
size_t ws_bytes_of(const Geom& g, bool h) {
  Sizer s;
  carve(s, g, h);
  return s.bytes();
}

unsigned stream_blocks(long long units) {   // grid-stride element-wise passes: ~4 units per thread, at most 2048 workgroups
  const int64_t b = ceil_div(units, 256 * 4);
  return static_cast<unsigned>(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

template <class F, int MODE>
void launch_gemm(const Gemm<F>& g, bool vec, bool b32, unsigned splits, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(ceil_div(g.m, kBM)), static_cast<unsigned>(ceil_div(g.n, kBN)), splits);
  if constexpr (F::k16 && (MODE == kFwdTrain || MODE == kFwdEval)) {   // an fp32 master weight under 16-bit rows
    if (b32) {
      if (vec) hipLaunchKernelGGL((lbn_gemm_k<F, MODE, true, true>), grid, dim3(256), 0, st, g);
      else hipLaunchKernelGGL((lbn_gemm_k<F, MODE, false, true>), grid, dim3(256), 0, st, g);
      return;
    }
  }
  if (vec) hipLaunchKernelGGL((lbn_gemm_k<F, MODE, true, false>), grid, dim3(256), 0, st, g);
  else hipLaunchKernelGGL((lbn_gemm_k<F, MODE, false, false>), grid, dim3(256), 0, st, g);
}

// dt: 0 (fp32 rows: wd and pd are 0 too) or one of the 16-bit formats, checked by the caller
template <class Fn>
int by_format(int dt, Fn fn) { return dt == 0 ? fn(G32{}) : dt == FV2P_DT_F16 ? fn(MH{}) : fn(MB{}); }
template <class F>
const typename F::elem* rd(const void* p) { return static_cast<const typename F::elem*>(p); }
template <class F>
typename F::elem* wr(void* p) { return static_cast<typename F::elem*>(p); }
template <class F>
bool vec_ok(int width) { return width % F::kVec == 0; }

// The arguments of the entry points, fp32 (`h` false; dt = wd = pd = 0) and _h alike; `who` is the entry point's name.
struct FwdArgs {
  const char* who; bool h;
  const void* x; int64_t n; int cin; const void* w; int cout; float eps, momentum; const void* gamma; const void* beta; int relu;
  void* running_mean; void* running_var; int64_t* nbt; void* z; float* mean; float* invstd; void* y; int dt, wd, pd;
  void* ws; size_t ws_bytes; fv2p_stream_t stream;
};
struct EvalArgs {
  const char* who; bool h;
  const void* x; int64_t n; int cin; const void* w; int cout; const float* mean; const float* invstd; const void* gamma; const void* beta;
  int relu; void* z; void* y; int dt, wd, pd; fv2p_stream_t stream;
};
struct BwdArgs {
  const char* who; bool h;
  const void* x; const void* z; const void* dy; int64_t n; int cin; const void* w; int cout; const float* mean; const float* invstd;
  const void* gamma; const void* beta; int relu, batch_stats; void* du; void* dx; void* dw; void* dgamma; void* dbeta; int dt, wd, pd;
  void* ws; size_t ws_bytes; fv2p_stream_t stream;
};

#define LBN_SHAPE(a)                                                                                                                          \
  FV2P_REQUIRE(shape_ok(a.n, a.cin, a.cout), FV2P_EINVAL, "%s: n %lld (1 .. 2^31 - 1), cin %d (1 .. %d), cout %d (1 .. %d)", a.who, (long long)a.n, \
               a.cin, kMaxCin, a.cout, kMaxCout)
#define LBN_FORMATS(a)                                                                                                                        \
  FV2P_REQUIRE(!a.h || formats_ok(a.dt, a.wd, a.pd), FV2P_EINVAL,                                                                             \
               "%s: dtype %d is neither fp16 (1) nor bf16 (2), or weight dtype %d / parameter dtype %d is neither 0 (fp32) nor the rows' dtype", a.who, \
               a.dt, a.wd, a.pd)
#define LBN_WORKSPACE(a, gm)                                                                                                                  \
  FV2P_REQUIRE(a.ws_bytes >= ws_bytes_of(gm, a.h), FV2P_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed", a.who, a.ws_bytes, ws_bytes_of(gm, a.h))

int forward(const FwdArgs& a) {
  LBN_SHAPE(a);
  FV2P_REQUIRE(a.n >= 2, FV2P_EINVAL, "%s: batch statistics of a single row", a.who);
  LBN_FORMATS(a);
  FV2P_REQUIRE(a.x && a.w && a.z && a.mean && a.invstd && a.y && a.ws, FV2P_EINVAL, "%s: null pointer", a.who);
  FV2P_REQUIRE((a.running_mean == nullptr) == (a.running_var == nullptr), FV2P_EINVAL, "%s: running_mean and running_var come together", a.who);
  const Geom gm = geom(a.n, a.cin, a.cout);
  LBN_WORKSPACE(a, gm);
  Carver cv(a.ws, a.ws_bytes);
  const Ws wsp = carve(cv, gm, a.h);
  hipStream_t st = static_cast<hipStream_t>(a.stream);
  return by_format(a.dt, [&](auto f) {
    using F = decltype(f);
    Gemm<F> g = {};
    g.a = a.x; g.lda = a.cin; g.b = a.w; g.ldb = a.cin;
    g.m = a.n; g.n = a.cout; g.k = a.cin;
    g.out = wr<F>(a.z); g.part = wsp.stats;
    launch_gemm<F, kFwdTrain>(g, vec_ok<F>(a.cin) && aligned16(a.x) && aligned16(a.w), a.wd == 0, 1, st);
    FV2P_LAUNCH_CHECK();
    const BnFwdFin ff{a.mean, a.invstd, nullptr, nullptr, reinterpret_cast<long long*>(a.nbt), a.momentum, a.eps};
    hipLaunchKernelGGL((lbn_fold_k<F, false>), dim3(static_cast<unsigned>(ceil_div(a.cout, F::kFoldCols))), dim3(256), 0, st, wsp.stats,
                       static_cast<int>(gm.row_tiles), static_cast<long long>(a.n), a.cout, ff, a.running_mean, a.running_var,
                       static_cast<void*>(nullptr), static_cast<void*>(nullptr), static_cast<float*>(nullptr), 1, a.pd);
    FV2P_LAUNCH_CHECK();
    long long* bump = a.running_mean ? reinterpret_cast<long long*>(a.nbt) : nullptr;
    const bool vec = vec_ok<F>(a.cout) && aligned16(a.z) && aligned16(a.y);
    const long long units = a.n * a.cout / (vec ? F::kVec : 1);
    const dim3 grid(stream_blocks(units));
    if (vec) hipLaunchKernelGGL((lbn_apply_k<F, F::kVec>), grid, dim3(256), 0, st, rd<F>(a.z), units, a.cout, a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu, wr<F>(a.y), bump);
    else hipLaunchKernelGGL((lbn_apply_k<F, 1>), grid, dim3(256), 0, st, rd<F>(a.z), units, a.cout, a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu, wr<F>(a.y), bump);
    FV2P_LAUNCH_CHECK();
    return 0;
  });
}

int forward_eval(const EvalArgs& a) {
  LBN_SHAPE(a);
  LBN_FORMATS(a);
  FV2P_REQUIRE(a.x && a.w && a.mean && a.invstd && a.y, FV2P_EINVAL, "%s: null pointer", a.who);
  return by_format(a.dt, [&](auto f) {
    using F = decltype(f);
    Gemm<F> g = {};
    g.a = a.x; g.lda = a.cin; g.b = a.w; g.ldb = a.cin;
    g.m = a.n; g.n = a.cout; g.k = a.cin;
    g.out = wr<F>(a.z); g.y = wr<F>(a.y);
    g.mean = a.mean; g.invstd = a.invstd; g.gamma = a.gamma; g.beta = a.beta; g.pd = a.pd; g.relu = a.relu;
    launch_gemm<F, kFwdEval>(g, vec_ok<F>(a.cin) && aligned16(a.x) && aligned16(a.w), a.wd == 0, 1, static_cast<hipStream_t>(a.stream));
    FV2P_LAUNCH_CHECK();
    return 0;
  });
}

int backward(const BwdArgs& a) {
  LBN_SHAPE(a);
  LBN_FORMATS(a);
  FV2P_REQUIRE(a.z && a.dy && a.mean && a.invstd && a.du && a.ws && (!a.dx || a.w) && (!a.dw || a.x), FV2P_EINVAL, "%s: null pointer", a.who);
  const int cin = a.cin, cout = a.cout;
  const int64_t n = a.n;
  const Geom gm = geom(n, cin, cout);
  LBN_WORKSPACE(a, gm);
  Carver cv(a.ws, a.ws_bytes);
  const Ws wsp = carve(cv, gm, a.h);
  hipStream_t st = static_cast<hipStream_t>(a.stream);
  return by_format(a.dt, [&](auto f) {
    using F = decltype(f);
    const typename F::elem* z = rd<F>(a.z);
    const typename F::elem* dy = rd<F>(a.dy);
    typename F::elem* du = wr<F>(a.du);
    const bool vec = vec_ok<F>(cout) && aligned16(z) && aligned16(dy) && aligned16(du);
    const dim3 rg(static_cast<unsigned>(gm.red_blocks));
    if (vec && F::kSumVec > 1) hipLaunchKernelGGL((lbn_bwd_sums_k<F, F::kSumVec>), rg, dim3(256), 0, st, z, dy, static_cast<long long>(n), cout,
                                                  static_cast<long long>(gm.red_rpb), a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu, wsp.stats);
    else hipLaunchKernelGGL((lbn_bwd_sums_k<F, 1>), rg, dim3(256), 0, st, z, dy, static_cast<long long>(n), cout, static_cast<long long>(gm.red_rpb),
                            a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu, wsp.stats);
    FV2P_LAUNCH_CHECK();
    hipLaunchKernelGGL((lbn_fold_k<F, true>), dim3(static_cast<unsigned>(ceil_div(cout, F::kFoldCols))), dim3(256), 0, st, wsp.stats,
                       static_cast<int>(gm.red_blocks), static_cast<long long>(n), cout, BnFwdFin{nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f},
                       static_cast<void*>(nullptr), static_cast<void*>(nullptr), a.dgamma, a.dbeta, wsp.coef, a.batch_stats, a.pd);
    FV2P_LAUNCH_CHECK();
    const long long units = n * cout / (vec ? F::kVec : 1);
    const dim3 grid(stream_blocks(units));
    if (vec) hipLaunchKernelGGL((lbn_du_k<F, F::kVec>), grid, dim3(256), 0, st, z, dy, units, cout, a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu, wsp.coef, du);
    else hipLaunchKernelGGL((lbn_du_k<F, 1>), grid, dim3(256), 0, st, z, dy, units, cout, a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu, wsp.coef, du);
    FV2P_LAUNCH_CHECK();
    const bool gvec = vec_ok<F>(cin) && vec_ok<F>(cout) && aligned16(du);
    if (a.dx) {   // dx [n][cin] = du [n][cout] * w [cout][cin]
      Gemm<F> g = {};
      g.a = du; g.lda = cout;
      g.m = n; g.n = cin; g.k = cout;
      g.out = wr<F>(a.dx);
      bool dvec;
      if constexpr (F::k16) {   // ... through wt [cin][cout]
        const dim3 tg(static_cast<unsigned>(ceil_div(cin, 32)), static_cast<unsigned>(ceil_div(cout, 32)));
        if (a.wd == 0) hipLaunchKernelGGL((lbn_wt_k<F, true>), tg, dim3(256), 0, st, a.w, cout, cin, wsp.wt);
        else hipLaunchKernelGGL((lbn_wt_k<F, false>), tg, dim3(256), 0, st, a.w, cout, cin, wsp.wt);
        FV2P_LAUNCH_CHECK();
        g.b = wsp.wt; g.ldb = cout;
        dvec = vec_ok<F>(cout) && aligned16(du) && aligned16(wsp.wt);
      } else {
        g.b = a.w; g.ldb = cin;
        dvec = gvec && aligned16(a.w);
      }
      launch_gemm<F, kData>(g, dvec, false, 1, st);
      FV2P_LAUNCH_CHECK();
    }
    if (a.dw) {   // dw [cout][cin] = sum over the rows of du [row][cout] * x [row][cin]
      Gemm<F> g = {};
      g.a = du; g.lda = cout; g.b = a.x; g.ldb = cin;
      g.m = cout; g.n = cin; g.k = n;
      g.part = wsp.wpart; g.chunk = gm.chunk;
      launch_gemm<F, kWeights>(g, gvec && aligned16(a.x), false, static_cast<unsigned>(gm.splits), st);
      FV2P_LAUNCH_CHECK();
      const long long elems = static_cast<long long>(cout) * cin;
      const dim3 fg(static_cast<unsigned>(ceil_div(elems, 256)));
      const bool w16 = F::k16 && a.wd != 0;   // a weight in T gets its gradient in T
      if constexpr (F::k16) {
        if (w16) hipLaunchKernelGGL((lbn_dw_fold_k<F, false>), fg, dim3(256), 0, st, wsp.wpart, gm.splits, elems, a.dw);
      }
      if (!w16) hipLaunchKernelGGL((lbn_dw_fold_k<F, true>), fg, dim3(256), 0, st, wsp.wpart, gm.splits, elems, a.dw);
      FV2P_LAUNCH_CHECK();
    }
    return 0;
  });
}

}  // namespace
}  // namespace fv2p

using namespace fv2p;

extern "C" int fv2p_linear_bn_h_supported(int64_t n, int cin, int cout, int dt, int wd, int pd) {
  return shape_ok(n, cin, cout) && formats_ok(dt, wd, pd) ? 1 : 0;
}

extern "C" size_t fv2p_linear_bn_ws_bytes(int64_t n, int cin, int cout) { return shape_ok(n, cin, cout) ? ws_bytes_of(geom(n, cin, cout), false) : 0; }
extern "C" size_t fv2p_linear_bn_h_ws_bytes(int64_t n, int cin, int cout) { return shape_ok(n, cin, cout) ? ws_bytes_of(geom(n, cin, cout), true) : 0; }
extern "C" int fv2p_linear_bn_splits(int64_t n, int cin, int cout) { return shape_ok(n, cin, cout) ? geom(n, cin, cout).splits : 0; }
extern "C" int fv2p_linear_bn_h_splits(int64_t n, int cin, int cout) { return fv2p_linear_bn_splits(n, cin, cout); }

extern "C" int fv2p_linear_bn_pays(int64_t n, int cin, int cout) {
  // forward + backward against the chunked rocBLAS product + fv2p_batchnorm_* at n = 49 152 (tools/microbench.py linbn,
  // profiles/linear_bn.txt): ahead by more than the larger spread at 16 > 128 (135 against 173 us), 128 > 128 (152 / 167 and 151 / 163)
  // and 32 > 160 (161 / 175); level at 64 > 192 (167 / 171); behind at 160 > 128 (183 / 163) and at the eight wider layers
  // (256 > 256: 353 / 301), where the backward pass pays for du written once and read by two GEMMs.  An earlier run on another machine
  // of the pool had the library route 40 - 60 us slower at the 128- and 192-wide layers and put 64 > 192 and 160 > 128 ahead as well;
  // they are not claimed.  Only that row count has been measured, so the claim holds for the octave around it and for those channel
  // pairs alone.
  static const int kPairs[][2] = {{16, 128}, {128, 128}, {32, 160}};
  if (n < 32768 || n > 65536) return 0;
  for (const auto& p : kPairs)
    if (cin == p[0] && cout == p[1]) return 1;
  return 0;
}

extern "C" int fv2p_linear_bn_h_pays(int64_t n, int cin, int cout, int dt) {
  // Filled from tools/microbench.py linbn16 (profiles/linear_bn_half.txt, n = 49 152): a shape pays where forward + backward is below
  // the route 16-bit rows take without this op (run_rows: the library's 16-bit product + fv2p_batchnorm_*_h) by more than the larger
  // spread of the windows.  Every channel pair of the decoder and BEVGridPooling's compression did, in both formats and in both runs
  // of the table (112 - 223 us against 202 - 346 us); at this row count both routes are bound by the host's calls, not by the GPU
  // (the op's kernels sum to about 120 us per forward + backward: profiles/linear_bn_half_kernel_stats.txt), so what is measured is
  // mostly the op's shorter sequence of calls.  Only that row count has been measured: the claim holds for the octave around it and
  // for those channel pairs alone.
  static const int kPairs[][2] = {{128, 256}, {256, 256}, {64, 192}, {192, 192}, {256, 192}, {32, 160}, {160, 160}, {192, 160},
                                  {16, 128}, {128, 128}, {160, 128}, {512, 128}};
  if (!dt_ok(dt) || n < 32768 || n > 65536) return 0;
  for (const auto& p : kPairs)
    if (cin == p[0] && cout == p[1]) return 1;
  return 0;
}

extern "C" int fv2p_linear_bn_forward(const float* x, int64_t n, int cin, const float* w, int cout, float eps, float momentum,
                                      const float* gamma, const float* beta, int relu, float* running_mean, float* running_var,
                                      int64_t* num_batches_tracked, float* z, float* mean, float* invstd, float* y, void* ws, size_t ws_bytes,
                                      fv2p_stream_t stream) {
  return forward({"fv2p_linear_bn_forward", false, x, n, cin, w, cout, eps, momentum, gamma, beta, relu, running_mean, running_var,
                  num_batches_tracked, z, mean, invstd, y, 0, 0, 0, ws, ws_bytes, stream});
}
extern "C" int fv2p_linear_bn_forward_h(const void* x, int64_t n, int cin, const void* w, int cout, float eps, float momentum,
                                        const void* gamma, const void* beta, int relu, void* running_mean, void* running_var,
                                        int64_t* num_batches_tracked, void* z, float* mean, float* invstd, void* y, int dt, int wd, int pd,
                                        void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  return forward({"fv2p_linear_bn_forward_h", true, x, n, cin, w, cout, eps, momentum, gamma, beta, relu, running_mean, running_var,
                  num_batches_tracked, z, mean, invstd, y, dt, wd, pd, ws, ws_bytes, stream});
}

extern "C" int fv2p_linear_bn_forward_eval(const float* x, int64_t n, int cin, const float* w, int cout, const float* mean,
                                           const float* invstd, const float* gamma, const float* beta, int relu, float* z, float* y,
                                           fv2p_stream_t stream) {
  return forward_eval({"fv2p_linear_bn_forward_eval", false, x, n, cin, w, cout, mean, invstd, gamma, beta, relu, z, y, 0, 0, 0, stream});
}
extern "C" int fv2p_linear_bn_forward_eval_h(const void* x, int64_t n, int cin, const void* w, int cout, const float* mean,
                                             const float* invstd, const void* gamma, const void* beta, int relu, void* z, void* y, int dt,
                                             int wd, int pd, fv2p_stream_t stream) {
  return forward_eval({"fv2p_linear_bn_forward_eval_h", true, x, n, cin, w, cout, mean, invstd, gamma, beta, relu, z, y, dt, wd, pd, stream});
}

extern "C" int fv2p_linear_bn_backward(const float* x, const float* z, const float* dy, int64_t n, int cin, const float* w, int cout,
                                       const float* mean, const float* invstd, const float* gamma, const float* beta, int relu,
                                       int batch_stats, float* du, float* dx, float* dw, float* dgamma, float* dbeta, void* ws,
                                       size_t ws_bytes, fv2p_stream_t stream) {
  return backward({"fv2p_linear_bn_backward", false, x, z, dy, n, cin, w, cout, mean, invstd, gamma, beta, relu, batch_stats, du, dx, dw,
                   dgamma, dbeta, 0, 0, 0, ws, ws_bytes, stream});
}
extern "C" int fv2p_linear_bn_backward_h(const void* x, const void* z, const void* dy, int64_t n, int cin, const void* w, int cout,
                                         const float* mean, const float* invstd, const void* gamma, const void* beta, int relu,
                                         int batch_stats, void* du, void* dx, void* dw, void* dgamma, void* dbeta, int dt, int wd, int pd,
                                         void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  return backward({"fv2p_linear_bn_backward_h", true, x, z, dy, n, cin, w, cout, mean, invstd, gamma, beta, relu, batch_stats, du, dx, dw,
                   dgamma, dbeta, dt, wd, pd, ws, ws_bytes, stream});
}
