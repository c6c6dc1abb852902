// Fused sparse convolution on 16-bit operands (fp16 / bf16) for gfx950: fv2p_sparse_conv_rows_h and fv2p_sparse_conv_wgrad_h
// (include/fv2p_ops.h).  Same contracts as the fp32 entry points of sparse_conv.hip, which this file does not touch: operands and
// results are stored in 16 bits, products run on v_mfma_f32_16x16x32_{f16,bf16} with fp32 accumulators, every sum has a fixed
// order (ascending k inside one workgroup / ascending row chunks), there are no atomics, and a result is rounded to 16 bits once.
//
// Operand maps of the 16x16x32 MFMA (wave64): lane l holds A[row l&15][k = 8(l>>4) + j] and B[k = 8(l>>4) + j][col l&15], j = 0..7,
// i.e. both operands want 8 CONSECUTIVE contraction indices in one 16-byte register group; C/D is col = l&15, row = 4(l>>4) + reg.
//   row conv : the contraction runs over source channels.  A gathered source row is contiguous in them, so the A fragment is one
//              16-byte global load per lane and 32 channels, no LDS.  The weight slice W_k goes through LDS as [c_dst][c_src]
//              (contraction contiguous): a plain copy for transpose_w = 1, a 4 x 8 register transpose for transpose_w = 0.
//   wgrad    : the contraction runs over rulebook pairs, along which BOTH operands are strided, so 32 gathered source rows and
//              their 32 gradient rows are staged through LDS transposed ([channel][pair]) with the same 4 x 8 register transpose.
// Channel counts that are not a multiple of 8 break the 16-byte alignment of rows: they take the element-wise, zero-filled fetch
// of the same kernels (template parameter AL = false).  No tensor is converted to fp32 anywhere.
//
// fv2p_sparse_conv_rows_hw32 / fv2p_sparse_conv_wgrad_hw32 are the same kernels for fp32 MASTER weights beside 16-bit rows (template
// parameter W32): the weight slice is read as fp32 and rounded to nearest even on its way into LDS - from LDS onward nothing differs,
// so the result has the bits of the 16-bit entry point on weight.to(dtype) - the fp32 bias joins the fp32 accumulator unrounded, and
// the reduce pass of the weight gradient stores its fp32 sum instead of rounding it.  These entry points make no 16-bit copy of the weights in memory.
#include <type_traits>

#include "common.hpp"

namespace fv2p {
namespace {

using u16 = unsigned short;
using f32x4 = float __attribute__((ext_vector_type(4)));
using f16x8 = _Float16 __attribute__((ext_vector_type(8)));
using bf16x8 = __bf16 __attribute__((ext_vector_type(8)));

struct F16 {
  static __device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ float widen(u16 v) { return static_cast<float>(__builtin_bit_cast(_Float16, v)); }
  static __device__ __forceinline__ u16 round(float v) { return __builtin_bit_cast(u16, static_cast<_Float16>(v)); }   // v_cvt_f16_f32: nearest even
};
struct BF16 {
  static __device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ float widen(u16 v) { return __uint_as_float(static_cast<unsigned>(v) << 16); }
  static __device__ __forceinline__ u16 round(float v) {   // nearest even on the upper 16 bits; NaN stays a (quiet) NaN
    const unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return static_cast<u16>((u >> 16) | 0x40u);
    return static_cast<u16>((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  }
};

__device__ __forceinline__ uint4 zero4() { return make_uint4(0u, 0u, 0u, 0u); }
__device__ __forceinline__ uint4 load16(const u16* p) { return *reinterpret_cast<const uint4*>(p); }
// 8 consecutive fp32 values (two 16-byte loads) rounded to T: the 16-byte group load16 would have read from the rounded tensor
template <class T>
__device__ __forceinline__ uint4 load16_round(const float* p) {
  const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
  const auto pack = [](float a, float b) { return static_cast<unsigned>(T::round(a)) | (static_cast<unsigned>(T::round(b)) << 16); };
  return make_uint4(pack(lo.x, lo.y), pack(lo.z, lo.w), pack(hi.x, hi.y), pack(hi.z, hi.w));
}
__device__ __forceinline__ unsigned word_of(const uint4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// r[i] = 8 consecutive 16-bit elements of row i (i = 0..3).  Column j of the 4 x 8 block, rows 0..3 packed into 8 bytes.
__device__ __forceinline__ uint2 column_of(const uint4 (&r)[4], int j) {
  const int w = j >> 1, sh = (j & 1) * 16;
  const unsigned e0 = (word_of(r[0], w) >> sh) & 0xffffu, e1 = (word_of(r[1], w) >> sh) & 0xffffu;
  const unsigned e2 = (word_of(r[2], w) >> sh) & 0xffffu, e3 = (word_of(r[3], w) >> sh) & 0xffffu;
  return make_uint2(e0 | (e1 << 16), e2 | (e3 << 16));
}

// 8 elements from p[0..7], those at or past `valid` read as zero (rows whose length is not a multiple of 8)
__device__ __forceinline__ uint4 load8_tail(const u16* p, int valid) {
  unsigned w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned lo = (2 * i < valid) ? p[2 * i] : 0u, hi = (2 * i + 1 < valid) ? p[2 * i + 1] : 0u;
    w[i] = lo | (hi << 16);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// ---------------------------------------------------------------- row conv --------------------------------------------------
constexpr int kRowGroups = 2;                        // 16-row groups per wave
constexpr int kTileRows = 4 * kRowGroups * 16;       // destination rows per workgroup
constexpr int kSlice = 64;                           // source channels of one staged weight slice
constexpr int kWld = kSlice + 8;                     // LDS row stride of a slice in elements (144 B: 16-byte aligned rows)

struct RowsArgs {
  const u16* src;
  const void* weight;   // 16-bit elements, or fp32 ones for the W32 kernels
  const int* tab;
  const void* bias;     // as weight
  u16* dst;
  int n_dst, c_src, c_dst, kvol, flip;
  int d0, cdn;   // this launch's destination columns [d0, d0 + cdn), cdn <= 128
};

// W_k[s0 .. s0 + 32 ksn)[d0 .. d0 + 16 NB) -> ws[c_dst][c_src] (zero outside the weight: an A fragment's zero fill must not meet
// whatever bits LDS held).  WT: the parameter is read as W_k^T, i.e. stored [K][c_dst][c_src].  W32: the parameter is fp32 and is
// rounded to T here, element by element, before the register transpose.
template <class T, int NB, bool WT, bool AL, bool W32>
__device__ __forceinline__ void stage_weight(u16* __restrict__ ws, const RowsArgs& a, int k, int s0, int ksn) {
  const int t = threadIdx.x;
  using W = std::conditional_t<W32, float, u16>;
  const W* __restrict__ wk = static_cast<const W*>(a.weight) + static_cast<long long>(k) * a.c_src * a.c_dst;
  const auto load8 = [](const W* p) {
    if constexpr (W32) return load16_round<T>(p); else return load16(p);
  };
  if constexpr (AL && WT) {
    const int chunks = ksn * 4, total = NB * 16 * chunks;
    for (int c = t; c < total; c += 256) {
      const int cd = c / chunks, cs = s0 + (c % chunks) * 8;
      const uint4 v = (cd < a.cdn && cs < a.c_src) ? load8(wk + static_cast<long long>(a.d0 + cd) * a.c_src + cs) : zero4();
      *reinterpret_cast<uint4*>(ws + cd * kWld + (cs - s0)) = v;
    }
  } else if constexpr (AL) {
    constexpr int cdg = NB * 2;
    const int total = ksn * 8 * cdg;
    for (int b = t; b < total; b += 256) {
      const int cd = (b % cdg) * 8, q = b / cdg, cs = s0 + q * 4;
      uint4 r[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        r[i] = (cs + i < a.c_src && cd < a.cdn) ? load8(wk + static_cast<long long>(cs + i) * a.c_dst + a.d0 + cd) : zero4();
#pragma unroll
      for (int j = 0; j < 8; ++j) *reinterpret_cast<uint2*>(ws + (cd + j) * kWld + q * 4) = column_of(r, j);
    }
  } else {
    constexpr int cdp = NB * 16;
    const int csp = ksn * 32;
    for (int e = t; e < cdp * csp; e += 256) {
      const int cd = WT ? e / csp : e % cdp, cs = WT ? e % csp : e / cdp;
      u16 v = 0;
      if (cd < a.cdn && s0 + cs < a.c_src) {
        const W e1 = WT ? wk[static_cast<long long>(a.d0 + cd) * a.c_src + s0 + cs] : wk[static_cast<long long>(s0 + cs) * a.c_dst + a.d0 + cd];
        if constexpr (W32) v = T::round(e1); else v = e1;
      }
      ws[cd * kWld + cs] = v;
    }
  }
}

template <class T, int NB, bool WT, bool AL, bool W32>
__global__ __launch_bounds__(256) void conv_rows_h(RowsArgs a) {
  __shared__ __align__(16) u16 ws[2][NB * 16 * kWld];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const long long row0 = static_cast<long long>(blockIdx.x) * kTileRows + wave * (kRowGroups * 16);
  f32x4 acc[kRowGroups][NB];
#pragma unroll
  for (int g = 0; g < kRowGroups; ++g)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[g][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int slices = (a.c_src + kSlice - 1) / kSlice;
  int buf = 0;
  for (int k = 0; k < a.kvol; ++k) {
    const int* __restrict__ trow = a.tab + static_cast<long long>(a.flip ? a.kvol - 1 - k : k) * a.n_dst;
    int idx[kRowGroups];
    bool any[kRowGroups];
#pragma unroll
    for (int g = 0; g < kRowGroups; ++g) {
      const long long r = row0 + g * 16 + lr;
      idx[g] = r < a.n_dst ? trow[r] : -1;
      any[g] = __ballot(idx[g] >= 0) != 0ull;   // no row of the group has a neighbour at this offset: its MFMAs are skipped
    }
    for (int sc = 0; sc < slices; ++sc, buf ^= 1) {
      const int s0 = sc * kSlice;
      const int csn = a.c_src - s0 < kSlice ? a.c_src - s0 : kSlice;
      const int ksn = (csn + 31) >> 5;
      uint4 afr[kRowGroups][2];
#pragma unroll
      for (int g = 0; g < kRowGroups; ++g)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const int ch = s0 + ks * 32 + lq * 8;
          afr[g][ks] = zero4();
          if (idx[g] >= 0 && ch < a.c_src) {
            const u16* p = a.src + static_cast<long long>(idx[g]) * a.c_src + ch;
            afr[g][ks] = AL ? load16(p) : load8_tail(p, a.c_src - ch);
          }
        }
      // two slices in LDS: the barrier below also says that every wave is done with the slice before last, whose place this one takes
      stage_weight<T, NB, WT, AL, W32>(ws[buf], a, k, s0, ksn);
      __syncthreads();
      bool wave_any = false;
#pragma unroll
      for (int g = 0; g < kRowGroups; ++g) wave_any |= any[g];
      if (!wave_any) continue;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        if (ks >= ksn) continue;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {   // one B fragment serves the wave's row groups
          const uint4 bfr = *reinterpret_cast<const uint4*>(&ws[buf][(nb * 16 + lr) * kWld + ks * 32 + lq * 8]);
#pragma unroll
          for (int g = 0; g < kRowGroups; ++g)
            if (any[g]) acc[g][nb] = T::mfma(afr[g][ks], bfr, acc[g][nb]);
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < kRowGroups; ++g)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int c = nb * 16 + lr;
      if (c >= a.cdn) continue;
      float b = 0.f;
      if (a.bias) {
        if constexpr (W32) b = static_cast<const float*>(a.bias)[a.d0 + c];   // joins the fp32 sum as it is: one rounding, at the store
        else b = T::widen(static_cast<const u16*>(a.bias)[a.d0 + c]);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const long long r = row0 + g * 16 + lq * 4 + reg;
        if (r < a.n_dst) a.dst[r * a.c_dst + a.d0 + c] = T::round(acc[g][nb][reg] + b);
      }
    }
}

// ---------------------------------------------------------------- weight gradient ---------------------------------------------
constexpr int kStep = 32;          // pairs per MFMA step (the 16x16x32 contraction)
constexpr int kSld = kStep + 8;    // LDS row stride of a staged step in elements (80 B: 16-byte aligned rows)

struct WgradArgs {
  const u16* src;
  const u16* grad;
  const int* tab;
  void* dw;   // 16-bit elements, or fp32 ones (F32 reduce pass)
  int n_dst, c_src, c_dst, kvol, flip;
  int s0, csn, d0, cdn;   // this launch's block of dW: source channels [s0, s0 + csn), gradient columns [d0, d0 + cdn), each <= 128
  int rpc;                // rows per chunk (a multiple of 256)
};

// pairs [p0, p0 + 32) of the chunk's list -> st[channel][pair]: rows 0 .. 16 MB - 1 the gathered source rows' channels, then the
// gradient rows' columns; zero past the list's end and past the channel counts
template <int MB, int NB, bool AL>
__device__ __forceinline__ void stage_pairs(u16* __restrict__ st, const WgradArgs& a, const int* __restrict__ list, int p0, int np) {
  const int t = threadIdx.x;
  if constexpr (AL) {
    constexpr int groups = (MB + NB) * 2;
    for (int b = t; b < groups * 8; b += 256) {
      const int cg = b % groups, q = b / groups;
      const bool is_src = cg < MB * 2;
      const int ch = (is_src ? cg : cg - MB * 2) * 8;
      const bool in = ch < (is_src ? a.csn : a.cdn);
      uint4 r[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = p0 + q * 4 + i;
        r[i] = zero4();
        if (in && p < np) {
          const long long row = list[2 * p + (is_src ? 0 : 1)];
          r[i] = load16(is_src ? a.src + row * a.c_src + a.s0 + ch : a.grad + row * a.c_dst + a.d0 + ch);
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) *reinterpret_cast<uint2*>(st + (cg * 8 + j) * kSld + q * 4) = column_of(r, j);
    }
  } else {
    constexpr int chans = (MB + NB) * 16;
    for (int e = t; e < chans * kStep; e += 256) {
      const int c = e % chans, q = e / chans, p = p0 + q;
      const bool is_src = c < MB * 16;
      const int ch = is_src ? c : c - MB * 16;
      u16 v = 0;
      if (p < np && ch < (is_src ? a.csn : a.cdn)) {
        const long long row = list[2 * p + (is_src ? 0 : 1)];
        v = is_src ? a.src[row * a.c_src + a.s0 + ch] : a.grad[row * a.c_dst + a.d0 + ch];
      }
      st[c * kSld + q] = v;
    }
  }
}

// One workgroup = one chunk of destination rows x one kernel offset: compacts the chunk's pairs of that offset (ascending row), walks
// them 32 at a time and leaves the fp32 tile [csn][cdn] in partial[chunk][k].
template <class T, int MB, int NB, bool AL>
__global__ __launch_bounds__(256) void conv_wgrad_h(WgradArgs a, float* __restrict__ partial) {
  extern __shared__ int list[];   // [rpc][2]: source row, gradient row
  __shared__ __align__(16) u16 st[2][(MB + NB) * 16 * kSld];
  __shared__ int scan[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int chunk = blockIdx.x, k = blockIdx.y;
  const int* __restrict__ trow = a.tab + static_cast<long long>(a.flip ? a.kvol - 1 - k : k) * a.n_dst;
  const long long r0 = static_cast<long long>(chunk) * a.rpc;
  int np = 0;
  for (int base = 0; base < a.rpc; base += 256) {
    const long long r = r0 + base + t;
    const int s = r < a.n_dst ? trow[r] : -1;
    int total;
    const int pos = block_excl_scan_256(s >= 0 ? 1 : 0, scan, &total);
    if (s >= 0) {
      list[2 * (np + pos)] = s;
      list[2 * (np + pos) + 1] = static_cast<int>(r);
    }
    np += total;
  }
  __syncthreads();
  constexpr int tiles = MB * NB, per_wave = tiles >= 4 ? tiles / 4 : 1;
  f32x4 acc[per_wave];
#pragma unroll
  for (int i = 0; i < per_wave; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  int buf = 0;
  for (int p0 = 0; p0 < np; p0 += kStep, buf ^= 1) {
    stage_pairs<MB, NB, AL>(st[buf], a, list, p0, np);
    __syncthreads();   // two steps in LDS: also says that every wave is done with the step before last
#pragma unroll
    for (int i = 0; i < per_wave; ++i) {
      const int tile = wave * per_wave + i;
      if (tile >= tiles) continue;
      const int mb = tile / NB, nb = tile % NB;
      const uint4 afr = *reinterpret_cast<const uint4*>(&st[buf][(mb * 16 + lr) * kSld + lq * 8]);
      const uint4 bfr = *reinterpret_cast<const uint4*>(&st[buf][((MB + nb) * 16 + lr) * kSld + lq * 8]);
      acc[i] = T::mfma(afr, bfr, acc[i]);
    }
  }
  float* __restrict__ out = partial + (static_cast<long long>(chunk) * a.kvol + k) * a.csn * a.cdn;
#pragma unroll
  for (int i = 0; i < per_wave; ++i) {
    const int tile = wave * per_wave + i;
    if (tile >= tiles) continue;
    const int cd = (tile % NB) * 16 + lr;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int cs = (tile / NB) * 16 + lq * 4 + reg;
      if (cs < a.csn && cd < a.cdn) out[cs * a.cdn + cd] = acc[i][reg];
    }
  }
}

// dW block = chunk partials summed in ascending chunk order, rounded once - or, F32, stored as the fp32 sum it is
template <class T, bool F32>
__global__ __launch_bounds__(256) void wgrad_reduce_h(const float* __restrict__ partial, int chunks, int kvol, int csn, int cdn, void* __restrict__ dw,
                                                      int c_src, int c_dst, int s0, int d0) {
  const long long per_chunk = static_cast<long long>(kvol) * csn * cdn;
  const long long e = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= per_chunk) return;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += partial[c * per_chunk + e];
  const int cd = static_cast<int>(e % cdn), cs = static_cast<int>((e / cdn) % csn), k = static_cast<int>(e / (static_cast<long long>(cdn) * csn));
  const long long o = (static_cast<long long>(k) * c_src + s0 + cs) * c_dst + d0 + cd;
  if constexpr (F32) static_cast<float*>(dw)[o] = s; else static_cast<u16*>(dw)[o] = T::round(s);
}

int pad_blocks(int blocks) { return blocks <= 1 ? 1 : blocks <= 2 ? 2 : blocks <= 4 ? 4 : 8; }
template <int N> using Blocks = std::integral_constant<int, N>;
template <class F> void for_blocks(int padded, F&& f) {
  switch (padded) { case 1: f(Blocks<1>{}); break; case 2: f(Blocks<2>{}); break; case 4: f(Blocks<4>{}); break; default: f(Blocks<8>{}); }
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <class T, bool WT, bool AL, bool W32>
void launch_rows(const RowsArgs& a, hipStream_t stream) {
  const dim3 grid(static_cast<unsigned>(ceil_div(a.n_dst, kTileRows))), block(256);
  for_blocks(pad_blocks(static_cast<int>(ceil_div(a.cdn, 16))), [&](auto nb) {
    hipLaunchKernelGGL((conv_rows_h<T, decltype(nb)::value, WT, AL, W32>), grid, block, 0, stream, a);
  });
}
template <class T, bool W32>
void launch_rows(const RowsArgs& a, bool wt, bool al, hipStream_t stream) {
  if (wt) { if (al) launch_rows<T, true, true, W32>(a, stream); else launch_rows<T, true, false, W32>(a, stream); }
  else    { if (al) launch_rows<T, false, true, W32>(a, stream); else launch_rows<T, false, false, W32>(a, stream); }
}

int wgrad_rows_per_chunk(int64_t n_dst) { return n_dst <= 32768 ? 512 : n_dst <= 131072 ? 1024 : 2048; }

template <class T, bool AL, bool F32>
void launch_wgrad(const WgradArgs& a, float* partial, unsigned chunks, hipStream_t stream) {
  const dim3 grid(chunks, static_cast<unsigned>(a.kvol)), block(256);
  const size_t lds = static_cast<size_t>(a.rpc) * 2 * sizeof(int);
  for_blocks(pad_blocks(static_cast<int>(ceil_div(a.csn, 16))), [&](auto mb) {
    for_blocks(pad_blocks(static_cast<int>(ceil_div(a.cdn, 16))), [&](auto nb) {
      hipLaunchKernelGGL((conv_wgrad_h<T, decltype(mb)::value, decltype(nb)::value, AL>), grid, block, lds, stream, a, partial);
    });
  });
  const long long per_chunk = static_cast<long long>(a.kvol) * a.csn * a.cdn;
  hipLaunchKernelGGL((wgrad_reduce_h<T, F32>), dim3(static_cast<unsigned>(ceil_div(per_chunk, 256))), block, 0, stream, partial, static_cast<int>(chunks),
                     a.kvol, a.csn, a.cdn, a.dw, a.c_src, a.c_dst, a.s0, a.d0);
}

// The two row-conv entry points: `name` is the one the caller used (it opens every message), W32 says that weight and bias are fp32.
template <bool W32>
int conv_rows_entry(const char* name, const void* src, int64_t n_src, int c_src, const void* weight, int kvol, const int* tab, int64_t n_dst, int c_dst,
                    int flip_k, int transpose_w, const void* bias, void* dst, int dtype, fv2p_stream_t stream_) {
  FV2P_DT16_OK(name, dtype);
  FV2P_REQUIRE(c_src >= 1 && c_dst >= 1 && kvol >= 1 && n_dst >= 0 && n_src >= 0, FV2P_EINVAL, "%s: bad sizes", name);
  if (n_dst == 0) return 0;
  FV2P_REQUIRE(weight && tab && dst && (src || n_src == 0), FV2P_EINVAL, "%s: null pointer", name);
  FV2P_REQUIRE(n_dst < (1ll << 31) - kTileRows, FV2P_ELIMIT, "%s: too many rows", name);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  RowsArgs a;
  a.src = static_cast<const u16*>(src); a.weight = weight; a.tab = tab;
  a.bias = bias; a.dst = static_cast<u16*>(dst);
  a.n_dst = static_cast<int>(n_dst); a.c_src = c_src; a.c_dst = c_dst; a.kvol = kvol; a.flip = flip_k & FV2P_TAB_FLIP;
  const bool al = c_src % 8 == 0 && c_dst % 8 == 0 && aligned16(src) && aligned16(weight);
  for (int d0 = 0; d0 < c_dst; d0 += 128) {   // every launch sums over ALL source channels: one rounding per element whatever c_src
    a.d0 = d0; a.cdn = c_dst - d0 < 128 ? c_dst - d0 : 128;
    if (dtype == FV2P_DT_F16) launch_rows<F16, W32>(a, transpose_w != 0, al, stream);
    else launch_rows<BF16, W32>(a, transpose_w != 0, al, stream);
  }
  FV2P_LAUNCH_CHECK();
  return 0;
}

size_t wgrad_ws_bytes(int64_t n_dst, int c_src, int c_dst, int kvol) {
  const int64_t n = n_dst > 0 ? n_dst : 1;
  const int cd = c_dst < 128 ? c_dst : 128, cs = c_src < 128 ? c_src : 128;
  Sizer s;
  s.take<float>(static_cast<size_t>(ceil_div(n, wgrad_rows_per_chunk(n_dst))) * (kvol > 0 ? kvol : 1) * (cs > 0 ? cs : 1) * (cd > 0 ? cd : 1));
  return s.bytes();
}

// The two weight-gradient entry points: F32 says that dweight is fp32 (the reduce pass then does not round).
template <bool F32>
int conv_wgrad_entry(const char* name, const void* src, int64_t n_src, int c_src, const void* grad, const int* tab, int64_t n_dst, int c_dst, int kvol,
                     int flip_k, void* dweight, int dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  FV2P_DT16_OK(name, dtype);
  FV2P_REQUIRE(c_src >= 1 && c_dst >= 1 && kvol >= 1 && n_dst >= 0 && n_src >= 0, FV2P_EINVAL, "%s: bad sizes", name);
  if (n_dst == 0) return 0;
  FV2P_REQUIRE(dweight && (src || n_src == 0) && grad && tab, FV2P_EINVAL, "%s: null pointer", name);
  FV2P_REQUIRE(n_dst < (1ll << 31) - 4096, FV2P_ELIMIT, "%s: too many rows", name);
  FV2P_REQUIRE(ws && ws_bytes >= wgrad_ws_bytes(n_dst, c_src, c_dst, kvol), FV2P_EWORKSPACE, "%s: workspace too small", name);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  WgradArgs a;
  a.src = static_cast<const u16*>(src); a.grad = static_cast<const u16*>(grad); a.tab = tab; a.dw = dweight;
  a.n_dst = static_cast<int>(n_dst); a.c_src = c_src; a.c_dst = c_dst; a.kvol = kvol; a.flip = flip_k & FV2P_TAB_FLIP;
  a.rpc = wgrad_rows_per_chunk(n_dst);
  const unsigned chunks = static_cast<unsigned>(ceil_div(n_dst, a.rpc));
  const bool al = c_src % 8 == 0 && c_dst % 8 == 0 && aligned16(src) && aligned16(grad);
  float* partial = static_cast<float*>(ws);
  for (int d0 = 0; d0 < c_dst; d0 += 128)
    for (int s0 = 0; s0 < c_src; s0 += 128) {   // blocks of dW are disjoint: the workspace is reused, launches are ordered by the stream
      a.d0 = d0; a.cdn = c_dst - d0 < 128 ? c_dst - d0 : 128;
      a.s0 = s0; a.csn = c_src - s0 < 128 ? c_src - s0 : 128;
      if (dtype == FV2P_DT_F16) { if (al) launch_wgrad<F16, true, F32>(a, partial, chunks, stream); else launch_wgrad<F16, false, F32>(a, partial, chunks, stream); }
      else                      { if (al) launch_wgrad<BF16, true, F32>(a, partial, chunks, stream); else launch_wgrad<BF16, false, F32>(a, partial, chunks, stream); }
    }
  FV2P_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace fv2p

using namespace fv2p;

extern "C" int fv2p_sparse_conv_rows_h(const void* src, int64_t n_src, int c_src, const void* weight, int kvol, const int* tab, int64_t n_dst,
                                       int c_dst, int flip_k, int transpose_w, const void* bias, void* dst, int dtype, fv2p_stream_t stream) {
  return conv_rows_entry<false>("sparse_conv_rows_h", src, n_src, c_src, weight, kvol, tab, n_dst, c_dst, flip_k, transpose_w, bias, dst, dtype, stream);
}

extern "C" int fv2p_sparse_conv_rows_hw32(const void* src, int64_t n_src, int c_src, const float* weight, int kvol, const int* tab, int64_t n_dst,
                                          int c_dst, int flip_k, int transpose_w, const float* bias, void* dst, int dtype, fv2p_stream_t stream) {
  return conv_rows_entry<true>("sparse_conv_rows_hw32", src, n_src, c_src, weight, kvol, tab, n_dst, c_dst, flip_k, transpose_w, bias, dst, dtype, stream);
}

extern "C" size_t fv2p_sparse_conv_wgrad_h_ws_bytes(int64_t n_dst, int c_src, int c_dst, int kvol) { return wgrad_ws_bytes(n_dst, c_src, c_dst, kvol); }

extern "C" int fv2p_sparse_conv_wgrad_h(const void* src, int64_t n_src, int c_src, const void* grad, const int* tab, int64_t n_dst, int c_dst,
                                        int kvol, int flip_k, void* dweight, int dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  return conv_wgrad_entry<false>("sparse_conv_wgrad_h", src, n_src, c_src, grad, tab, n_dst, c_dst, kvol, flip_k, dweight, dtype, ws, ws_bytes, stream);
}

extern "C" int fv2p_sparse_conv_wgrad_hw32(const void* src, int64_t n_src, int c_src, const void* grad, const int* tab, int64_t n_dst, int c_dst,
                                           int kvol, int flip_k, float* dweight, int dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  return conv_wgrad_entry<true>("sparse_conv_wgrad_hw32", src, n_src, c_src, grad, tab, n_dst, c_dst, kvol, flip_k, dweight, dtype, ws, ws_bytes, stream);
}
