// nn.Linear(bias=False) -> nn.BatchNorm1d [-> nn.ReLU] over float16 / bfloat16 point rows: the 16-bit sibling of linear_bn.hip (the
// thirteen layers of the voxel-to-point decoder and BEVGridPooling's compression after .half(), .bfloat16() or under autocast).
//
// Arithmetic contract.  T is float16 or bfloat16 (dt), u its unit roundoff.  x [n][cin] in T; w [cout][cin] in T or fp32 (wd); an fp32
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
//                       operand.  dx = du * w: fp32 accumulators, one rounding to T.  dw = du^T * x over a fixed split of the rows: the
//                       fp32 MFMA accumulators cover at most 128 rows before they are added into fp64 sums, the partial tiles are
//                       folded in split order and rounded once (to_odd, then T::round) into a T weight, or stored as fp32 for an fp32
//                       master weight.  dgamma / dbeta in the parameters' format.
//   5. determinism      no float atomics, no workgroup waits for another, no fp32 copy of any [n, .] tensor: bit-identical results
//                       from run to run.
//
// One tile GEMM serves the four products (lbnh_gemm_k), as in the fp32 op: a workgroup of four waves owns 128 output rows x 64 output
// columns, wave v the rows 32 v .. 32 v + 31 as 2 x 4 tiles of 16 x 16.  Both operands lie in LDS as [row][k] images of 64 K values
// (row stride 72 elements: 16-byte aligned; the 16-byte K groups of a row are permuted by (row / 8) % 8 so that the transposing stores
// of the weight-gradient pass spread over the banks), read as one 16-byte fragment per lane and MFMA: lane l holds
// A[l & 15][8 (l >> 4) + j] and B[8 (l >> 4) + j][l & 15]; D[4 (l >> 4) + r][l & 15] comes back in register r.  The next chunk's
// global loads are issued before this chunk's MFMAs.
//   forward            x and w are K-contiguous: 16-byte global loads, 16-byte LDS stores
//   backward data      w^T is materialised in T in the workspace per call (lbnh_wt_k: <= 1 MB; it also rounds an fp32 master weight),
//                      so the product has the forward's form
//   backward weights   K = rows, neither operand K-contiguous: 16-byte loads along the channels of two rows, and the pair of rows goes
//                      into the [channel][row] image as one 32-bit LDS store per channel
// Ragged extents on all three dimensions are zero-filled on load (branch-free guarded loads) and never stored; cin or cout not a
// multiple of 8, or a base that is not 16-byte aligned, takes the element-wise load path.
#include <algorithm>

#include "common.hpp"
#include "bn_fold.hpp"

namespace fv2p {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
using f16x8 = _Float16 __attribute__((ext_vector_type(8)));
using bf16x8 = __bf16 __attribute__((ext_vector_type(8)));

struct MH : H16 {
  static __device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};
struct MB : B16 {
  static __device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};

constexpr int kBM = 128;          // output rows per workgroup (the A operand's side): 4 waves x 32
constexpr int kBN = 64;           // output columns per workgroup (the B operand's side)
constexpr int kKC = 64;           // K per LDS chunk: two MFMA steps of 32
constexpr int kLd = kKC + 8;      // elements per image row
constexpr int kFlush = 2;         // backward weights: K chunks (128 rows) between two additions into the fp64 sums
constexpr int kMaxCin = 1024, kMaxCout = 512;
constexpr int kFoldCols = 8, kFoldLanes = 32;   // the fold kernels: 8 columns x 32 interleaved row lanes per workgroup
constexpr int kSumUnits = 32, kSumLanes = 8;    // backward BatchNorm sums: 32 units of 8 (or 1) columns x 8 row lanes at a time
constexpr int kRedRows = 64;      // backward BatchNorm sums: at least this many rows per workgroup
constexpr int kRedBlocks = 1024;  // ... and at most this many workgroups
constexpr int64_t kWgBytes = 16ll << 20;   // backward weights: at most this many bytes of fp64 partial tiles

enum Mode { kFwdTrain, kFwdEval, kData, kWeights };

struct Gemm {
  const void* a;    // M side operand (T)
  const void* b;    // N side operand (T; fp32 where the kernel's B32 says so)
  long long lda, ldb;
  long long m, n, k;      // output rows, output columns, length of the sum
  u16* out;               // [m][n]: z (may be null in eval mode) or dx
  double* part;           // kFwdTrain: [row tiles][2][n] sums; kWeights: [splits][m][n] partial tiles
  long long chunk;        // kWeights: K per split (a multiple of kFlush * kKC)
  const float* mean; const float* invstd; const void* gamma; const void* beta; int pd;   // kFwdEval
  int relu;
  u16* y;
};

// element offset of (row, k) in a [ROWS][kLd] image: the 16-byte K groups of a row are permuted by (row / 8) % 8
__device__ __forceinline__ int img(int row, int k) { return row * kLd + ((((k >> 3) ^ (row >> 3)) & 7) << 3) + (k & 7); }

// Guarded loads without a branch (head1x1.hip): an address that is always readable and the value 0 outside.
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

// A thread's share of a ROWS x kKC operand tile: NV units of 8 elements, along K (KCONT) or along the rows.
// Element (row, k) of the operand is p[row * ld + k] (KCONT) or p[k * ld + row].  SRC32: the operand is fp32 in memory (KCONT only).
// Units along the rows come in pairs (2 j, 2 j + 1) = rows k, k + 1 of the same 8 channels.
template <class T, int ROWS, bool KCONT, bool VEC, bool SRC32>
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
  // into the image s[ROWS][kLd]
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

template <class T, int MODE, bool VEC, bool B32>
__global__ __launch_bounds__(256) void lbnh_gemm_k(const Gemm g) {
  constexpr bool KCONT = MODE != kWeights;
  __shared__ __attribute__((aligned(16))) u16 as[kBM * kLd];
  __shared__ __attribute__((aligned(16))) u16 bs[kBN * kLd];
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
  Tile<T, kBM, KCONT, VEC, false> ta;
  Tile<T, kBN, KCONT, VEC, B32> tb;
  ta.load(g.a, g.lda, m0, g.m, k_begin, k_end);
  tb.load(g.b, g.ldb, n0, g.n, k_begin, k_end);
  int since = 0;
  for (long long k0 = k_begin; k0 < k_end; k0 += kKC) {
    __syncthreads();
    ta.store(as);
    tb.store(bs);
    __syncthreads();
    // the next chunk's loads fly during this one's MFMAs (past k_end they are guarded away)
    ta.load(g.a, g.lda, m0, g.m, k0 + kKC, k_end);
    tb.load(g.b, g.ldb, n0, g.n, k0 + kKC, k_end);
#pragma unroll
    for (int ks = 0; ks < kKC / 32; ++ks) {
      uint4 av[2], bv[4];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) av[mi] = *reinterpret_cast<const uint4*>(as + img(wave * 32 + mi * 16 + li, 32 * ks + 8 * lk));
#pragma unroll
      for (int nj = 0; nj < 4; ++nj) bv[nj] = *reinterpret_cast<const uint4*>(bs + img(nj * 16 + li, 32 * ks + 8 * lk));
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nj = 0; nj < 4; ++nj) acc[mi][nj] = T::mfma(av[mi], bv[nj], acc[mi][nj]);
    }
    if constexpr (MODE == kWeights) {
      if (++since == kFlush) { flush(); since = 0; }
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
      const float mu = g.mean[e], is = g.invstd[e], ga = par_load<T>(g.gamma, e, g.pd, 1.f), be = par_load<T>(g.beta, e, g.pd, 0.f);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long row = row_base + mi * 16 + r;
          if (row >= g.m) continue;
          const u16 zb = T::round(acc[mi][nj][r]);
          const float z = T::widen(zb);
          const float t = (z - mu) * is * ga + be;
          if (g.out) g.out[row * g.n + col] = zb;
          g.y[row * g.n + col] = T::round((g.relu && t <= 0.f) ? 0.f : t);   // NaN passes through, like torch.relu
        }
    }
  } else {
    // z (or dx) rounded once; the forward's sums below are those of the rounded values
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int nj = 0; nj < 4; ++nj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long row = row_base + mi * 16 + r, col = n0 + nj * 16 + li;
          const u16 zb = T::round(acc[mi][nj][r]);
          if (row < g.m && col < g.n) g.out[row * g.n + col] = zb;
          if constexpr (MODE == kFwdTrain) acc[mi][nj][r] = T::widen(zb);
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

// w [cout][cin] (T, or fp32 rounded once) -> wt [cin][cout] in T: the B operand of the backward data product
template <class T, bool W32>
__global__ __launch_bounds__(256) void lbnh_wt_k(const void* __restrict__ w, int cout, int cin, u16* __restrict__ wt) {
  __shared__ u16 tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int co = co0 + ty + 8 * j, ci = ci0 + tx;
    u16 v = 0;
    if (co < cout && ci < cin) {
      const long long e = static_cast<long long>(co) * cin + ci;
      if constexpr (W32) v = T::round(static_cast<const float*>(w)[e]);
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

// ---- fold of the [rows][2][c] partial sums: a workgroup takes 8 columns, 32 lanes per column walk interleaved rows, then an ordered
// LDS fold.  Forward: mean, invstd and the running statistics in the parameters' format (bn_fwd_channel); every column reads
// *num_batches_tracked (momentum=None) and nobody in this launch writes it: the apply launch that follows does.
// Backward: dbeta, dgamma (the parameters' format) and the two means of the input gradient (fp32). -----------------------------------
template <class T, bool BWD>
__global__ __launch_bounds__(256) void lbnh_fold_k(const double* __restrict__ part, int rows, long long n, int c, BnFwdFin ff, void* running_mean,
                                                   void* running_var, void* dgamma, void* dbeta, float* coef, int batch_stats, int pd) {
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
    bn_fwd_channel<Fmt16<T>>(a, b, n, ff, running_mean, running_var, pd, col, true, &mu, &is);
  } else {
    const double nn = static_cast<double>(n);
    if (dbeta) par_store<T>(dbeta, col, pd, a);
    if (dgamma) par_store<T>(dgamma, col, pd, b);
    coef[col] = batch_stats ? static_cast<float>(a / nn) : 0.f;
    coef[c + col] = batch_stats ? static_cast<float>(b / nn) : 0.f;
  }
}

// per-column constants of the element-wise passes, staged in LDS once per workgroup
struct Cols {
  float mean[kMaxCout], is[kMaxCout], gamma[kMaxCout], beta[kMaxCout];
};
template <class T>
__device__ __forceinline__ void cols_load(Cols& s, int c, const float* mean, const float* invstd, const void* gamma, const void* beta, int pd) {
  for (int e = threadIdx.x; e < c; e += 256) {
    s.mean[e] = mean[e];
    s.is[e] = invstd[e];
    s.gamma[e] = par_load<T>(gamma, e, pd, 1.f);
    s.beta[e] = par_load<T>(beta, e, pd, 0.f);
  }
}

// y = round_T(relu?((z - mean) * invstd * gamma + beta)); units of V elements (V = 8: c % 8 == 0).  The launch comes after the fold, so
// its first thread is the one that advances num_batches_tracked (null: not tracked).
template <class T, int V>
__global__ __launch_bounds__(256) void lbnh_apply_k(const u16* __restrict__ z, long long units, int c, const float* __restrict__ mean,
                                                    const float* __restrict__ invstd, const void* __restrict__ gamma,
                                                    const void* __restrict__ beta, int pd, int relu, u16* __restrict__ y, long long* nbt) {
  __shared__ Cols s;
  cols_load<T>(s, c, mean, invstd, gamma, beta, pd);
  __syncthreads();
  if (nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;
  const int cv = c / V;
  for (long long u = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; u < units; u += static_cast<long long>(gridDim.x) * 256) {
    const int col = static_cast<int>(u % cv) * V;
    Row16<T, V> zv, o;
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
// part[b][2][c].  32 units of V columns x 8 row lanes at a time (V = 8: c % 8 == 0, one 16-byte access per tensor and row); a thread
// sums its rows in row order, the row lanes are folded in lane order through LDS.
template <class T, int V>
__global__ __launch_bounds__(256) void lbnh_bwd_sums_k(const u16* __restrict__ z, const u16* __restrict__ dy, long long n, int c, long long rpb,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd,
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
        ga[i] = par_load<T>(gamma, col + i, pd, 1.f); be[i] = par_load<T>(beta, col + i, pd, 0.f);
      }
#pragma unroll 2
      for (long long r = r0 + rl; r < r1; r += kSumLanes) {
        Row16<T, V> zv, gv;
        zv.load(z + r * c + col);
        gv.load(dy + r * c + col);
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
    for (int e = tid; e < kSumUnits * V; e += 256) {
      if (c0 + e >= c) continue;
      double sa = 0.0, sb = 0.0;
      for (int q = 0; q < kSumLanes; ++q) { sa += red[0][q][e]; sb += red[1][q][e]; }
      part[(static_cast<long long>(blockIdx.x) * 2 + 0) * c + c0 + e] = sa;
      part[(static_cast<long long>(blockIdx.x) * 2 + 1) * c + c0 + e] = sb;
    }
  }
}

// du = round_T(gamma * invstd * (dz - c1 - xhat * c2)), the gradient of the pre-activation z (coef = [c1][c2], zeros for a frozen
// BatchNorm)
template <class T, int V>
__global__ __launch_bounds__(256) void lbnh_du_k(const u16* __restrict__ z, const u16* __restrict__ dy, long long units, int c,
                                                 const float* __restrict__ mean, const float* __restrict__ invstd, const void* __restrict__ gamma,
                                                 const void* __restrict__ beta, int pd, int relu, const float* __restrict__ coef,
                                                 u16* __restrict__ du) {
  __shared__ Cols s;
  __shared__ float c1[kMaxCout], c2[kMaxCout];
  cols_load<T>(s, c, mean, invstd, gamma, beta, pd);
  for (int e = threadIdx.x; e < c; e += 256) { c1[e] = coef[e]; c2[e] = coef[c + e]; }
  __syncthreads();
  const int cv = c / V;
  for (long long u = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; u < units; u += static_cast<long long>(gridDim.x) * 256) {
    const int col = static_cast<int>(u % cv) * V;
    Row16<T, V> zv, gv, o;
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

// dw[e] = the fp64 partials of element e summed in split order, one rounding at the store (fp32 for an fp32 master weight)
template <class T, bool W32>
__global__ __launch_bounds__(256) void lbnh_dw_fold_k(const double* __restrict__ part, int splits, long long elems, void* __restrict__ dw) {
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
  if constexpr (W32) static_cast<float*>(dw)[e] = static_cast<float>(acc);
  else static_cast<u16*>(dw)[e] = T::round(to_odd(acc));
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
  g.split_bound = std::min<int64_t>(ceil_div(n, kFlush * kKC), cap);
  g.chunk = ceil_div(ceil_div(n, g.split_bound), kFlush * kKC) * (kFlush * kKC);
  g.splits = static_cast<int>(ceil_div(n, g.chunk));
  return g;
}

struct Ws {
  double* stats;   // [max(row_tiles, red_blocks)][2][cout]
  float* coef;     // [2][cout]
  double* wpart;   // [splits][cout][cin]
  u16* wt;         // [cin][cout]
};
template <typename C>
Ws carve(C& cv, const Geom& g) {
  Ws w;
  w.stats = cv.template take<double>(static_cast<size_t>(std::max(g.row_tiles, g.red_blocks)) * 2 * g.cout);
  w.coef = cv.template take<float>(2 * static_cast<size_t>(g.cout));
  w.wpart = cv.template take<double>(static_cast<size_t>(g.split_bound) * g.cout * g.cin);
  w.wt = cv.template take<u16>(static_cast<size_t>(g.cout) * g.cin);
  return w;
}
size_t ws_bytes_of(const Geom& g) {
  Sizer s;
  carve(s, g);
  return s.bytes();
}

unsigned stream_blocks(long long units) {   // grid-stride element-wise passes: ~4 units per thread, at most 2048 workgroups
  const int64_t b = ceil_div(units, 256 * 4);
  return static_cast<unsigned>(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

template <class T, int MODE>
void launch_gemm(const Gemm& g, bool vec, bool b32, unsigned splits, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(ceil_div(g.m, kBM)), static_cast<unsigned>(ceil_div(g.n, kBN)), splits);
  if constexpr (MODE == kFwdTrain || MODE == kFwdEval) {
    if (b32) {
      if (vec) hipLaunchKernelGGL((lbnh_gemm_k<T, MODE, true, true>), grid, dim3(256), 0, st, g);
      else hipLaunchKernelGGL((lbnh_gemm_k<T, MODE, false, true>), grid, dim3(256), 0, st, g);
      return;
    }
  }
  if (vec) hipLaunchKernelGGL((lbnh_gemm_k<T, MODE, true, false>), grid, dim3(256), 0, st, g);
  else hipLaunchKernelGGL((lbnh_gemm_k<T, MODE, false, false>), grid, dim3(256), 0, st, g);
}

struct FwdArgs {
  const void* x; int64_t n; int cin; const void* w; int cout; float eps, momentum; const void* gamma; const void* beta; int relu;
  void* running_mean; void* running_var; int64_t* nbt; void* z; float* mean; float* invstd; void* y; int wd, pd;
};

template <class T>
int forward_run(const FwdArgs& a, const Geom& gm, const Ws& wsp, hipStream_t st) {
  Gemm g = {};
  g.a = a.x; g.lda = a.cin; g.b = a.w; g.ldb = a.cin;
  g.m = a.n; g.n = a.cout; g.k = a.cin;
  g.out = static_cast<u16*>(a.z); g.part = wsp.stats;
  launch_gemm<T, kFwdTrain>(g, a.cin % 8 == 0 && aligned16(a.x) && aligned16(a.w), a.wd == 0, 1, st);
  FV2P_LAUNCH_CHECK();
  const BnFwdFin ff{a.mean, a.invstd, nullptr, nullptr, reinterpret_cast<long long*>(a.nbt), a.momentum, a.eps};
  hipLaunchKernelGGL((lbnh_fold_k<T, false>), dim3(static_cast<unsigned>(ceil_div(a.cout, kFoldCols))), dim3(256), 0, st, wsp.stats,
                     static_cast<int>(gm.row_tiles), static_cast<long long>(a.n), a.cout, ff, a.running_mean, a.running_var,
                     static_cast<void*>(nullptr), static_cast<void*>(nullptr), static_cast<float*>(nullptr), 1, a.pd);
  FV2P_LAUNCH_CHECK();
  long long* bump = a.running_mean ? reinterpret_cast<long long*>(a.nbt) : nullptr;
  const bool vec = a.cout % 8 == 0 && aligned16(a.z) && aligned16(a.y);
  const long long units = a.n * a.cout / (vec ? 8 : 1);
  const u16* z = static_cast<const u16*>(a.z);
  u16* y = static_cast<u16*>(a.y);
  if (vec) hipLaunchKernelGGL((lbnh_apply_k<T, 8>), dim3(stream_blocks(units)), dim3(256), 0, st, z, units, a.cout, a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu, y, bump);
  else hipLaunchKernelGGL((lbnh_apply_k<T, 1>), dim3(stream_blocks(units)), dim3(256), 0, st, z, units, a.cout, a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu, y, bump);
  FV2P_LAUNCH_CHECK();
  return 0;
}

struct BwdArgs {
  const void* x; const void* z; const void* dy; int64_t n; int cin; const void* w; int cout; const float* mean; const float* invstd;
  const void* gamma; const void* beta; int relu, batch_stats; void* du; void* dx; void* dw; void* dgamma; void* dbeta; int wd, pd;
};

template <class T>
int backward_run(const BwdArgs& a, const Geom& gm, const Ws& wsp, hipStream_t st) {
  const int cin = a.cin, cout = a.cout;
  const int64_t n = a.n;
  const u16* z = static_cast<const u16*>(a.z);
  const u16* dy = static_cast<const u16*>(a.dy);
  u16* du = static_cast<u16*>(a.du);
  const bool vec = cout % 8 == 0 && aligned16(z) && aligned16(dy) && aligned16(du);
  const dim3 rg(static_cast<unsigned>(gm.red_blocks));
  if (vec) hipLaunchKernelGGL((lbnh_bwd_sums_k<T, 8>), rg, dim3(256), 0, st, z, dy, static_cast<long long>(n), cout, static_cast<long long>(gm.red_rpb),
                              a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu, wsp.stats);
  else hipLaunchKernelGGL((lbnh_bwd_sums_k<T, 1>), rg, dim3(256), 0, st, z, dy, static_cast<long long>(n), cout, static_cast<long long>(gm.red_rpb),
                          a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu, wsp.stats);
  FV2P_LAUNCH_CHECK();
  hipLaunchKernelGGL((lbnh_fold_k<T, true>), dim3(static_cast<unsigned>(ceil_div(cout, kFoldCols))), dim3(256), 0, st, wsp.stats,
                     static_cast<int>(gm.red_blocks), static_cast<long long>(n), cout, BnFwdFin{nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f},
                     static_cast<void*>(nullptr), static_cast<void*>(nullptr), a.dgamma, a.dbeta, wsp.coef, a.batch_stats, a.pd);
  FV2P_LAUNCH_CHECK();
  const long long units = n * cout / (vec ? 8 : 1);
  if (vec) hipLaunchKernelGGL((lbnh_du_k<T, 8>), dim3(stream_blocks(units)), dim3(256), 0, st, z, dy, units, cout, a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu, wsp.coef, du);
  else hipLaunchKernelGGL((lbnh_du_k<T, 1>), dim3(stream_blocks(units)), dim3(256), 0, st, z, dy, units, cout, a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu, wsp.coef, du);
  FV2P_LAUNCH_CHECK();
  if (a.dx) {   // dx [n][cin] = du [n][cout] * w [cout][cin], through wt [cin][cout]
    const dim3 tg(static_cast<unsigned>(ceil_div(cin, 32)), static_cast<unsigned>(ceil_div(cout, 32)));
    if (a.wd == 0) hipLaunchKernelGGL((lbnh_wt_k<T, true>), tg, dim3(256), 0, st, a.w, cout, cin, wsp.wt);
    else hipLaunchKernelGGL((lbnh_wt_k<T, false>), tg, dim3(256), 0, st, a.w, cout, cin, wsp.wt);
    FV2P_LAUNCH_CHECK();
    Gemm g = {};
    g.a = du; g.lda = cout; g.b = wsp.wt; g.ldb = cout;
    g.m = n; g.n = cin; g.k = cout;
    g.out = static_cast<u16*>(a.dx);
    launch_gemm<T, kData>(g, cout % 8 == 0 && aligned16(du) && aligned16(wsp.wt), false, 1, st);
    FV2P_LAUNCH_CHECK();
  }
  if (a.dw) {   // dw [cout][cin] = sum over the rows of du [row][cout] * x [row][cin]
    Gemm g = {};
    g.a = du; g.lda = cout; g.b = a.x; g.ldb = cin;
    g.m = cout; g.n = cin; g.k = n;
    g.part = wsp.wpart; g.chunk = gm.chunk;
    launch_gemm<T, kWeights>(g, cin % 8 == 0 && cout % 8 == 0 && aligned16(du) && aligned16(a.x), false, static_cast<unsigned>(gm.splits), st);
    FV2P_LAUNCH_CHECK();
    const long long elems = static_cast<long long>(cout) * cin;
    const dim3 fg(static_cast<unsigned>(ceil_div(elems, 256)));
    if (a.wd == 0) hipLaunchKernelGGL((lbnh_dw_fold_k<T, true>), fg, dim3(256), 0, st, wsp.wpart, gm.splits, elems, a.dw);
    else hipLaunchKernelGGL((lbnh_dw_fold_k<T, false>), fg, dim3(256), 0, st, wsp.wpart, gm.splits, elems, a.dw);
    FV2P_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace
}  // namespace fv2p

using namespace fv2p;

extern "C" int fv2p_linear_bn_h_supported(int64_t n, int cin, int cout, int dt, int wd, int pd) {
  return shape_ok(n, cin, cout) && formats_ok(dt, wd, pd) ? 1 : 0;
}

extern "C" size_t fv2p_linear_bn_h_ws_bytes(int64_t n, int cin, int cout) {
  if (!shape_ok(n, cin, cout)) return 0;
  return ws_bytes_of(geom(n, cin, cout));
}

extern "C" int fv2p_linear_bn_h_splits(int64_t n, int cin, int cout) {
  if (!shape_ok(n, cin, cout)) return 0;
  return geom(n, cin, cout).splits;
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

#define LBNH_SHAPE(who)                                                                                                                  \
  FV2P_REQUIRE(shape_ok(n, cin, cout), FV2P_EINVAL, who ": n %lld (1 .. 2^31 - 1), cin %d (1 .. %d), cout %d (1 .. %d)", (long long)n, cin, \
               kMaxCin, cout, kMaxCout)
#define LBNH_FORMATS(who)                                                                                                                \
  FV2P_REQUIRE(formats_ok(dt, wd, pd), FV2P_EINVAL, who ": dtype %d is neither fp16 (1) nor bf16 (2), or weight dtype %d / parameter dtype %d is neither 0 (fp32) nor the rows' dtype", \
               dt, wd, pd)

extern "C" int fv2p_linear_bn_forward_h(const void* x, int64_t n, int cin, const void* w, int cout, float eps, float momentum,
                                        const void* gamma, const void* beta, int relu, void* running_mean, void* running_var,
                                        int64_t* num_batches_tracked, void* z, float* mean, float* invstd, void* y, int dt, int wd, int pd,
                                        void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  LBNH_SHAPE("fv2p_linear_bn_forward_h");
  FV2P_REQUIRE(n >= 2, FV2P_EINVAL, "fv2p_linear_bn_forward_h: batch statistics of a single row");
  LBNH_FORMATS("fv2p_linear_bn_forward_h");
  FV2P_REQUIRE(x && w && z && mean && invstd && y && ws, FV2P_EINVAL, "fv2p_linear_bn_forward_h: null pointer");
  FV2P_REQUIRE((running_mean == nullptr) == (running_var == nullptr), FV2P_EINVAL, "fv2p_linear_bn_forward_h: running_mean and running_var come together");
  const Geom gm = geom(n, cin, cout);
  FV2P_REQUIRE(ws_bytes >= ws_bytes_of(gm), FV2P_EWORKSPACE, "fv2p_linear_bn_forward_h: workspace of %zu bytes, %zu needed", ws_bytes, ws_bytes_of(gm));
  Carver cv(ws, ws_bytes);
  const Ws wsp = carve(cv, gm);
  const FwdArgs a{x, n, cin, w, cout, eps, momentum, gamma, beta, relu, running_mean, running_var, num_batches_tracked, z, mean, invstd, y, wd, pd};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dt == FV2P_DT_F16 ? forward_run<MH>(a, gm, wsp, st) : forward_run<MB>(a, gm, wsp, st);
}

extern "C" int fv2p_linear_bn_forward_eval_h(const void* x, int64_t n, int cin, const void* w, int cout, const float* mean,
                                             const float* invstd, const void* gamma, const void* beta, int relu, void* z, void* y, int dt,
                                             int wd, int pd, fv2p_stream_t stream) {
  LBNH_SHAPE("fv2p_linear_bn_forward_eval_h");
  LBNH_FORMATS("fv2p_linear_bn_forward_eval_h");
  FV2P_REQUIRE(x && w && mean && invstd && y, FV2P_EINVAL, "fv2p_linear_bn_forward_eval_h: null pointer");
  Gemm g = {};
  g.a = x; g.lda = cin; g.b = w; g.ldb = cin;
  g.m = n; g.n = cout; g.k = cin;
  g.out = static_cast<u16*>(z); g.y = static_cast<u16*>(y);
  g.mean = mean; g.invstd = invstd; g.gamma = gamma; g.beta = beta; g.pd = pd; g.relu = relu;
  const bool vec = cin % 8 == 0 && aligned16(x) && aligned16(w);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dt == FV2P_DT_F16) launch_gemm<MH, kFwdEval>(g, vec, wd == 0, 1, st);
  else launch_gemm<MB, kFwdEval>(g, vec, wd == 0, 1, st);
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" int fv2p_linear_bn_backward_h(const void* x, const void* z, const void* dy, int64_t n, int cin, const void* w, int cout,
                                         const float* mean, const float* invstd, const void* gamma, const void* beta, int relu,
                                         int batch_stats, void* du, void* dx, void* dw, void* dgamma, void* dbeta, int dt, int wd, int pd,
                                         void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  LBNH_SHAPE("fv2p_linear_bn_backward_h");
  LBNH_FORMATS("fv2p_linear_bn_backward_h");
  FV2P_REQUIRE(z && dy && mean && invstd && du && ws && (!dx || w) && (!dw || x), FV2P_EINVAL, "fv2p_linear_bn_backward_h: null pointer");
  const Geom gm = geom(n, cin, cout);
  FV2P_REQUIRE(ws_bytes >= ws_bytes_of(gm), FV2P_EWORKSPACE, "fv2p_linear_bn_backward_h: workspace of %zu bytes, %zu needed", ws_bytes, ws_bytes_of(gm));
  Carver cv(ws, ws_bytes);
  const Ws wsp = carve(cv, gm);
  const BwdArgs a{x, z, dy, n, cin, w, cout, mean, invstd, gamma, beta, relu, batch_stats, du, dx, dw, dgamma, dbeta, wd, pd};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dt == FV2P_DT_F16 ? backward_run<MH>(a, gm, wsp, st) : backward_run<MB>(a, gm, wsp, st);
}
