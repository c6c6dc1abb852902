// Multi-head 1x1 convolution over an fp32 NCHW map with position-major outputs: the three 1x1 Conv2d of the anchor head
// (conv_cls, conv_box, conv_dir_cls of anchor_head_single.py:21-37, whose outputs forward() permutes to [B, H, W, Ck] :48-60).
//
//   forward          y_k[g][j]  = sum_c x[b][c][p] * W_k[j][c] + bias_k[j]          g = b * P + p, P = H * W
//   backward data    dx[b][c][p] = sum_k sum_j W_k[j][c] * dy_k[g][j]
//   backward weights dW_k[j][c]  = sum_g dy_k[g][j] * x[b][c][p],   db_k[j] = sum_g dy_k[g][j]
//
// The heads are concatenated along the output channel: n = off_k + j, sum Ck <= 64, padded to NB blocks of 16.  Forward and backward
// data run on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate over the channels / the columns), backward weights on
// v_mfma_f64_16x16x4_f64 (the sum over all positions of the batch).  The map is read and written as it stands in NCHW: for one channel
// consecutive positions are contiguous, so a lane moves 4 consecutive positions with one 16-byte access (VEC: P % 4 == 0 and 16-byte
// aligned maps; element by element otherwise) and the 4 components go to 4 different MFMA tiles - the K index (forward, backward
// weights) or the row index (backward data) of a tile is a permutation both operands share.
//
// MFMA operand layout (lane = 16 * lk + li): A[i = li][k = lk], B[k = lk][j = li], D[i = 4 * lk + r][j = li] in register r.
//
// No atomics anywhere: backward weights splits the positions over workgroups, every workgroup leaves its partial tile in the
// workspace (fp64) and a second small launch folds the partials in split order, so dW and db are bit-identical from run to run.
#include <algorithm>

#include "common.hpp"

namespace fv2p {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

struct H1 {
  const float* x;        // [B, Cin, P]
  float* dx;
  const float* w[3];     // [Ck, Cin]
  const float* bias[3];  // [Ck] or null
  float* y[3];           // [B * P, Ck]
  const float* dy[3];
  float* dw[3];
  float* db[3];          // may be null
  double* part;          // backward weights: [splits][np][cin] partial tiles, then [splits][4][64] partial bias sums
  int ck[3];
  int off[3];            // first concatenated column of head k
  int tot, np;           // sum Ck, padded to a multiple of 16
  int cin;
  int p, n;              // positions per sample, positions in all (B * P < 2^30)
  int splits, chunk;     // backward weights: workgroups along the positions, positions per workgroup (a multiple of the 32-position tile)
};

__device__ __forceinline__ int head_of(const H1& a, int n) { return n < a.off[1] ? 0 : (n < a.off[2] ? 1 : 2); }
template <typename T>
__device__ __forceinline__ T sel3(T const (&v)[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

// Guarded loads without a branch: the address is replaced by one that is always readable and the value by 0.  (A load inside a
// divergent branch is waited for where the branch joins, which serialises a run of guarded loads: one memory latency each.)
__device__ __forceinline__ float ld_or0(const float* p, bool ok, const float* safe) {
  const float v = *(ok ? p : safe);
  return ok ? v : 0.f;
}
__device__ __forceinline__ float4 ld4_or0(const float* p, bool ok, const float* safe) {
  const float4 v = *reinterpret_cast<const float4*>(ok ? p : safe);
  return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}

// W[n][c] of the concatenated weights, 0 outside [tot, cin)
__device__ __forceinline__ float wcat(const H1& a, int n, int c) {
  const bool ok = n < a.tot && c < a.cin;
  const int k = ok ? head_of(a, n) : 0;
  return ld_or0(sel3(a.w, k) + static_cast<long long>(n - sel3(a.off, k)) * a.cin + c, ok, a.w[0]);
}

constexpr int kFwdKC = 32;   // forward: channels per weight chunk in LDS
constexpr int kBwdCC = 64;   // backward data: channels per weight chunk in LDS

// ---- forward: a wave owns 64 positions x all columns, a workgroup 256 positions; the weights stream through LDS by K chunks -----------
template <int NB, bool VEC>
__global__ __launch_bounds__(256) void head1x1_fwd_k(const H1 a) {
  __shared__ __attribute__((aligned(16))) float wl[kFwdKC / 4 * 64 * NB];   // [K step][lane][nb]: B fragments in lane order
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int g0 = (blockIdx.x * 4 + wave) * 64;
  // row li of tile q is position g0 + 4 * li + q; xo[q]: its offset in x at channel 0, -1 outside the map
  long long xo[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int g = g0 + 4 * li + q;
    xo[q] = -1;
    if (g < a.n) {
      const int b = g / a.p;
      xo[q] = static_cast<long long>(b) * a.cin * a.p + (g - b * a.p);
    }
  }
  auto load = [&](int c) {
    const bool c_ok = c < a.cin;
    const long long co = static_cast<long long>(c) * a.p;
    if constexpr (VEC) {
      return ld4_or0(a.x + xo[0] + co, c_ok && xo[0] >= 0, a.x);
    } else {
      return make_float4(ld_or0(a.x + xo[0] + co, c_ok && xo[0] >= 0, a.x), ld_or0(a.x + xo[1] + co, c_ok && xo[1] >= 0, a.x),
                         ld_or0(a.x + xo[2] + co, c_ok && xo[2] >= 0, a.x), ld_or0(a.x + xo[3] + co, c_ok && xo[3] >= 0, a.x));
    }
  };
  f32x4 acc[4][NB];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[q][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  // a thread's share of a weight chunk: element e = tid + 256 * i is W[n = e / kFwdKC][c0 + e % kFwdKC] (rows read 128 bytes at a time)
  constexpr int WPT = kFwdKC * 16 * NB / 256;
  float4 xv[kFwdKC / 4], xn[kFwdKC / 4];
  float wr[WPT];
#pragma unroll
  for (int s = 0; s < kFwdKC / 4; ++s) xv[s] = load(4 * s + lk);
#pragma unroll
  for (int i = 0; i < WPT; ++i) wr[i] = wcat(a, (tid + 256 * i) / kFwdKC, (tid + 256 * i) % kFwdKC);
  for (int c0 = 0; c0 < a.cin; c0 += kFwdKC) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const int e = tid + 256 * i, n = e / kFwdKC, cc = e % kFwdKC;
      wl[((cc >> 2) * 64 + (cc & 3) * 16 + (n & 15)) * NB + (n >> 4)] = wr[i];
    }
    __syncthreads();
    // the next chunk's map and weight loads fly during this one's MFMAs
#pragma unroll
    for (int s = 0; s < kFwdKC / 4; ++s) xn[s] = load(c0 + kFwdKC + 4 * s + lk);
#pragma unroll
    for (int i = 0; i < WPT; ++i) wr[i] = wcat(a, (tid + 256 * i) / kFwdKC, c0 + kFwdKC + (tid + 256 * i) % kFwdKC);
#pragma unroll
    for (int s = 0; s < kFwdKC / 4; ++s) {
      float wv[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) wv[nb] = wl[(s * 64 + lane) * NB + nb];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        acc[0][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].x, wv[nb], acc[0][nb], 0, 0, 0);
        acc[1][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].y, wv[nb], acc[1][nb], 0, 0, 0);
        acc[2][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].z, wv[nb], acc[2][nb], 0, 0, 0);
        acc[3][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].w, wv[nb], acc[3][nb], 0, 0, 0);
      }
    }
#pragma unroll
    for (int s = 0; s < kFwdKC / 4; ++s) xv[s] = xn[s];
  }
  // D row 4 * lk + r of tile q is position g0 + 16 * lk + 4 * r + q; column li of block nb is n = 16 * nb + li
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int n = nb * 16 + li;
    if (n >= a.tot) continue;
    const int k = head_of(a, n), ck = sel3(a.ck, k), col = n - sel3(a.off, k);
    const float* bp = sel3(a.bias, k);
    const float bias = bp ? bp[col] : 0.f;
    float* yk = sel3(a.y, k) + col;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int g = g0 + 16 * lk + 4 * r + q;
        if (g < a.n) yk[static_cast<long long>(g) * ck] = acc[q][nb][r] + bias;
      }
  }
}

// ---- backward data: a wave owns 64 positions, keeps their dy rows as A fragments and walks the channels 16 at a time ----------------
template <int NB, bool VEC>
__global__ __launch_bounds__(256) void head1x1_bwd_data_k(const H1 a) {
  constexpr int KS = NB * 4;   // K steps of 4 concatenated columns
  __shared__ __attribute__((aligned(16))) float wl[(kBwdCC / 16) * KS * 64];   // [channel block][K step / 4][lane][K step % 4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int g0 = (blockIdx.x * 4 + wave) * 64;
  // A: row li of tile q is position g0 + 16 * q + li, k = lk is column n = 4 * s + lk
  float av[4][KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int n = 4 * s + lk;
    const bool col_ok = n < a.tot;
    const int k = col_ok ? head_of(a, n) : 0;
    const int ck = sel3(a.ck, k);
    const float* dp = sel3(a.dy, k) + (n - sel3(a.off, k));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int g = g0 + 16 * q + li;
      av[q][s] = ld_or0(dp + static_cast<long long>(g) * ck, col_ok && g < a.n, a.dy[0]);
    }
  }
  // D row 4 * lk + r of tile q is position g0 + 16 * q + 4 * lk + r (4 consecutive positions per lane), column li a channel
  long long xo[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int g = g0 + 16 * q + 4 * lk;
    xo[q] = -1;
    if (g < a.n) {
      const int b = g / a.p;
      xo[q] = static_cast<long long>(b) * a.cin * a.p + (g - b * a.p);
    }
  }
  // a thread's share of a weight chunk: element e = tid + 256 * i is W[n = e / kBwdCC][c0 + e % kBwdCC]; the next chunk's share is
  // loaded while this chunk's MFMAs run
  constexpr int WPT = 16 * NB * kBwdCC / 256;
  float wr[WPT];
#pragma unroll
  for (int i = 0; i < WPT; ++i) wr[i] = wcat(a, (tid + 256 * i) / kBwdCC, (tid + 256 * i) % kBwdCC);
  for (int c0 = 0; c0 < a.cin; c0 += kBwdCC) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const int e = tid + 256 * i, n = e / kBwdCC, cc = e % kBwdCC, s = n >> 2;
      wl[(((cc >> 4) * NB + (s >> 2)) * 64 + (n & 3) * 16 + (cc & 15)) * 4 + (s & 3)] = wr[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < WPT; ++i) wr[i] = wcat(a, (tid + 256 * i) / kBwdCC, c0 + kBwdCC + (tid + 256 * i) % kBwdCC);
#pragma unroll 1
    for (int cb = 0; cb < kBwdCC / 16; ++cb) {
      if (c0 + cb * 16 >= a.cin) break;
      f32x4 acc[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s4 = 0; s4 < NB; ++s4) {
        const float4 wv = *reinterpret_cast<const float4*>(&wl[((cb * NB + s4) * 64 + lane) * 4]);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q][4 * s4 + 0], wv.x, acc[q], 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q][4 * s4 + 1], wv.y, acc[q], 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q][4 * s4 + 2], wv.z, acc[q], 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q][4 * s4 + 3], wv.w, acc[q], 0, 0, 0);
      }
      const int c = c0 + cb * 16 + li;
      if (c >= a.cin) continue;
      const long long co = static_cast<long long>(c) * a.p;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if constexpr (VEC) {
          if (xo[q] >= 0) *reinterpret_cast<float4*>(a.dx + xo[q] + co) = make_float4(acc[q][0], acc[q][1], acc[q][2], acc[q][3]);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int g = g0 + 16 * q + 4 * lk + r;
            if (g < a.n) {
              const int b = g / a.p;
              a.dx[static_cast<long long>(b) * a.cin * a.p + (g - b * a.p) + co] = acc[q][r];
            }
          }
        }
      }
    }
  }
}

// ---- backward weights: workgroup (split, slab) = chunk positions x 64 channels; wave w owns channels 16 * w .. + 15 of the slab x all
// columns.  K = positions: a lane's 16-byte load of x holds the k = lk entries of 4 consecutive K steps.  The dy rows of a tile of positions
// are contiguous per head: the workgroup reads them with coalesced loads into LDS, transposed to [column][position], and every wave
// takes its A fragments from there, 4 K steps per 16-byte read.  Map and dy of the next tile are loaded during the MFMAs.
// The sum over B * H * W positions runs on v_mfma_f64_16x16x4_f64: the products of two floats are exact in fp64 and the accumulation
// loses nothing that shows in fp32, so dW is the correctly rounded sum (a float chain over 10^5 positions is not, and torch's own
// small-shape kernels accumulate in fp64 too).  A/B lanes as the f32 form; D[i = lk + 4 * r][j = li] in register pair r. ------------
constexpr int kWgU = 2;       // 16-position K blocks per LDS tile
constexpr int kWgTP = 16 * kWgU;   // positions per tile
constexpr int kWgLd = kWgTP + 4;   // floats per column row of the tile (16-byte reads stay aligned, rows on different banks)
template <int NB, bool VEC>
__global__ __launch_bounds__(256, 2) void head1x1_bwd_weights_k(const H1 a) {   // two waves per SIMD: 256 VGPRs
  __shared__ __attribute__((aligned(16))) float sdy[16 * NB * kWgLd];   // [column n][position of the tile]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int split = blockIdx.x, c = (blockIdx.y * 4 + wave) * 16 + li;
  const bool c_ok = c < a.cin;
  const bool bias_wave = blockIdx.y == 0 && wave == 0;
  const int begin = split * a.chunk, end = min(begin + a.chunk, a.n);
  // a thread's share of a dy tile: element e = tid + 256 * i of the heads' kWgTP-position blocks laid end to end, decoded once:
  // bit 31 valid, head << 28, position in the tile << 20, column n << 12, offset in the head's block
  constexpr int DPT = kWgTP * 16 * NB / 256;
  int meta[DPT];
#pragma unroll
  for (int i = 0; i < DPT; ++i) {
    const int e = tid + 256 * i;
    meta[i] = 0;
    if (e < kWgTP * a.tot) {
      const int k = e < kWgTP * a.off[1] ? 0 : (e < kWgTP * a.off[2] ? 1 : 2);
      const int idx = e - kWgTP * sel3(a.off, k), ck = sel3(a.ck, k), pos = idx / ck;
      meta[i] = static_cast<int>(0x80000000u | (k << 28) | (pos << 20) | ((sel3(a.off, k) + idx - pos * ck) << 12) | idx);
    }
  }
  auto dy_load = [&](int gs, float (&d)[DPT]) {
#pragma unroll
    for (int i = 0; i < DPT; ++i) {
      const int m = meta[i], k = (m >> 28) & 3;
      d[i] = ld_or0(sel3(a.dy, k) + static_cast<long long>(gs) * sel3(a.ck, k) + (m & 4095), m < 0 && gs + ((m >> 20) & 63) < end, a.dy[0]);
    }
  };
  auto x_load = [&](int gs, float4 (&xv)[kWgU]) {
#pragma unroll
    for (int u = 0; u < kWgU; ++u) {
      const int g = gs + 16 * u + 4 * lk;   // this lane's 4 positions: g .. g + 3
      if constexpr (VEC) {
        const int b = g / a.p;
        xv[u] = ld4_or0(a.x + (static_cast<long long>(b) * a.cin + c) * a.p + (g - b * a.p), c_ok && g < end, a.x);
      } else {
        float t[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int b = (g + q) / a.p;
          t[q] = ld_or0(a.x + (static_cast<long long>(b) * a.cin + c) * a.p + (g + q - b * a.p), c_ok && g + q < end, a.x);
        }
        xv[u] = make_float4(t[0], t[1], t[2], t[3]);
      }
    }
  };
  f64x4 acc[NB];
  double bsum[NB];   // (one wave of the launch: its cost does not show)
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) { acc[nb] = f64x4{0.0, 0.0, 0.0, 0.0}; bsum[nb] = 0.0; }
  for (int e = tid; e < 16 * NB * kWgLd; e += 256) sdy[e] = 0.f;   // the padded columns stay zero
  float4 xc[kWgU], xn[kWgU];
  float dn[DPT];
  x_load(begin, xc);
  dy_load(begin, dn);
  for (int gs = begin; gs < end; gs += 16 * kWgU) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < DPT; ++i)
      if (meta[i] < 0) sdy[((meta[i] >> 12) & 127) * kWgLd + ((meta[i] >> 20) & 63)] = dn[i];
    __syncthreads();
    x_load(gs + 16 * kWgU, xn);
    dy_load(gs + 16 * kWgU, dn);
#pragma unroll
    for (int u = 0; u < kWgU; ++u) {
      float4 av[NB];   // A[i = li][k = lk] of 4 K steps: column n = 16 * nb + li at positions 16 * u + 4 * lk ..+ 3 of the tile
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) av[nb] = *reinterpret_cast<const float4*>(&sdy[(nb * 16 + li) * kWgLd + 16 * u + 4 * lk]);
      // component by component, so that consecutive MFMAs go to different accumulators
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[nb].x, xc[u].x, acc[nb], 0, 0, 0);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[nb].y, xc[u].y, acc[nb], 0, 0, 0);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[nb].z, xc[u].z, acc[nb], 0, 0, 0);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[nb].w, xc[u].w, acc[nb], 0, 0, 0);
      if (bias_wave) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) bsum[nb] += (static_cast<double>(av[nb].x) + av[nb].y) + (static_cast<double>(av[nb].z) + av[nb].w);
      }
      __builtin_amdgcn_sched_barrier(0);   // one K block's fragments and fp64 operands live at a time
    }
#pragma unroll
    for (int u = 0; u < kWgU; ++u) xc[u] = xn[u];
  }
  // D[i = lk + 4 * r][j = li]: column n = 16 * nb + lk + 4 * r, channel c
  if (c_ok) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = nb * 16 + lk + 4 * r;
        a.part[(static_cast<long long>(split) * a.np + n) * a.cin + c] = acc[nb][r];
      }
  }
  if (bias_wave) {
    double* bpart = a.part + static_cast<long long>(a.splits) * a.np * a.cin;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) bpart[(split * 4 + lk) * 64 + nb * 16 + li] = bsum[nb];
  }
}

// the fp64 partials of one element summed in split order, one rounding at the store; the last `tot` threads take the bias sums
__global__ __launch_bounds__(256) void head1x1_fold_k(const H1 a) {
  const long long e = blockIdx.x * 256ll + threadIdx.x, nw = static_cast<long long>(a.tot) * a.cin;
  if (e < nw) {
    const int n = static_cast<int>(e / a.cin), c = static_cast<int>(e % a.cin);
    const double* p = a.part + static_cast<long long>(n) * a.cin + c;
    const long long stride = static_cast<long long>(a.np) * a.cin;
    double acc = 0.0;
    for (int s0 = 0; s0 < a.splits; s0 += 16) {
      double v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = s0 + i < a.splits ? p[(s0 + i) * stride] : 0.0;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc += v[i];
    }
    const int k = head_of(a, n);
    sel3(a.dw, k)[static_cast<long long>(n - sel3(a.off, k)) * a.cin + c] = static_cast<float>(acc);
  } else if (e < nw + a.tot) {
    const int n = static_cast<int>(e - nw), k = head_of(a, n);
    float* db = sel3(a.db, k);
    if (!db) return;
    const double* p = a.part + static_cast<long long>(a.splits) * a.np * a.cin + n;
    double acc = 0.0;
    for (int s = 0; s < a.splits * 4; ++s) acc += p[s * 64];
    db[n - sel3(a.off, k)] = static_cast<float>(acc);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
constexpr int64_t kMaxPos = 1ll << 30;   // positions and position + chunk stay in an int

// the shape both directions share; returns 0 or a negative code
int h1_geom(const char* who, int64_t b, int cin, int64_t hw, int c0, int c1, int c2, H1* a) {
  FV2P_REQUIRE(b >= 1 && cin >= 1 && hw >= 1, FV2P_EINVAL, "%s: empty map (b %lld, cin %d, hw %lld)", who, (long long)b, cin, (long long)hw);
  FV2P_REQUIRE(c0 >= 1 && c1 >= 0 && c2 >= 0 && (c2 == 0 || c1 > 0), FV2P_EINVAL, "%s: head widths (%d, %d, %d): heads are packed to the front",
               who, c0, c1, c2);
  FV2P_REQUIRE(c0 + c1 + c2 <= 64, FV2P_ELIMIT, "%s: %d output channels in all, at most 64", who, c0 + c1 + c2);
  FV2P_REQUIRE(hw < kMaxPos && b * hw < kMaxPos, FV2P_ELIMIT, "%s: %lld x %lld positions are more than 2^30", who, (long long)b, (long long)hw);
  a->ck[0] = c0; a->ck[1] = c1; a->ck[2] = c2;
  a->off[0] = 0; a->off[1] = c0; a->off[2] = c0 + c1;
  a->tot = c0 + c1 + c2;
  a->np = (a->tot + 15) / 16 * 16;
  a->cin = cin;
  a->p = static_cast<int>(hw);
  a->n = static_cast<int>(b * hw);
  const int slabs = (cin + 63) / 64;
  int64_t s = std::min<int64_t>(ceil_div(a->n, 256), ceil_div(768, slabs));   // 768 workgroups: three waves per SIMD take turns on the fp64 MFMA pipe while the others wait for their tile
  if (s < 1) s = 1;
  a->chunk = static_cast<int>(ceil_div(ceil_div(a->n, s), 16 * kWgU) * 16 * kWgU);
  a->splits = static_cast<int>(ceil_div(a->n, a->chunk));
  return 0;
}
size_t h1_ws_bytes(const H1& a) {
  Sizer s;
  s.take<double>(static_cast<size_t>(a.splits) * a.np * a.cin + static_cast<size_t>(a.splits) * 4 * 64);
  return s.bytes();
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

#define H1_DISPATCH(kernel, nb, vec, grid, stream, a)                                                      \
  do {                                                                                                     \
    switch ((nb) * 2 + ((vec) ? 1 : 0)) {                                                                  \
      case 2: hipLaunchKernelGGL((kernel<1, false>), grid, dim3(256), 0, stream, a); break;                \
      case 3: hipLaunchKernelGGL((kernel<1, true>), grid, dim3(256), 0, stream, a); break;                 \
      case 4: hipLaunchKernelGGL((kernel<2, false>), grid, dim3(256), 0, stream, a); break;                \
      case 5: hipLaunchKernelGGL((kernel<2, true>), grid, dim3(256), 0, stream, a); break;                 \
      case 6: hipLaunchKernelGGL((kernel<3, false>), grid, dim3(256), 0, stream, a); break;                \
      case 7: hipLaunchKernelGGL((kernel<3, true>), grid, dim3(256), 0, stream, a); break;                 \
      case 8: hipLaunchKernelGGL((kernel<4, false>), grid, dim3(256), 0, stream, a); break;                \
      default: hipLaunchKernelGGL((kernel<4, true>), grid, dim3(256), 0, stream, a); break;                \
    }                                                                                                      \
  } while (0)

}  // namespace
}  // namespace fv2p

using namespace fv2p;

extern "C" size_t fv2p_head1x1_ws_bytes(int64_t b, int cin, int64_t hw, int c0, int c1, int c2) {
  H1 a = {};
  if (h1_geom("fv2p_head1x1_ws_bytes", b, cin, hw, c0, c1, c2, &a) != 0) return 0;
  return h1_ws_bytes(a);
}

extern "C" int fv2p_head1x1_forward(const float* x, int64_t b, int cin, int64_t hw, const float* w0, const float* w1, const float* w2,
                                    const float* bias0, const float* bias1, const float* bias2, int c0, int c1, int c2, float* y0, float* y1,
                                    float* y2, fv2p_stream_t stream) {
  H1 a = {};
  if (int rc = h1_geom("fv2p_head1x1_forward", b, cin, hw, c0, c1, c2, &a)) return rc;
  FV2P_REQUIRE(x && w0 && y0 && (!c1 || (w1 && y1)) && (!c2 || (w2 && y2)), FV2P_EINVAL, "fv2p_head1x1_forward: null map, weight or output");
  a.x = x;
  a.w[0] = w0; a.w[1] = w1; a.w[2] = w2;
  a.bias[0] = bias0; a.bias[1] = bias1; a.bias[2] = bias2;
  a.y[0] = y0; a.y[1] = y1; a.y[2] = y2;
  const bool vec = a.p % 4 == 0 && aligned16(x);
  const dim3 grid(static_cast<unsigned>(ceil_div(a.n, 256)));
  H1_DISPATCH(head1x1_fwd_k, a.np / 16, vec, grid, static_cast<hipStream_t>(stream), a);
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" int fv2p_head1x1_backward_data(const float* dy0, const float* dy1, const float* dy2, int64_t b, int cin, int64_t hw, const float* w0,
                                          const float* w1, const float* w2, int c0, int c1, int c2, float* dx, fv2p_stream_t stream) {
  H1 a = {};
  if (int rc = h1_geom("fv2p_head1x1_backward_data", b, cin, hw, c0, c1, c2, &a)) return rc;
  FV2P_REQUIRE(dx && w0 && dy0 && (!c1 || (w1 && dy1)) && (!c2 || (w2 && dy2)), FV2P_EINVAL, "fv2p_head1x1_backward_data: null map, weight or gradient");
  a.dx = dx;
  a.w[0] = w0; a.w[1] = w1; a.w[2] = w2;
  a.dy[0] = dy0; a.dy[1] = dy1; a.dy[2] = dy2;
  const bool vec = a.p % 4 == 0 && aligned16(dx);
  const dim3 grid(static_cast<unsigned>(ceil_div(a.n, 256)));
  H1_DISPATCH(head1x1_bwd_data_k, a.np / 16, vec, grid, static_cast<hipStream_t>(stream), a);
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" int fv2p_head1x1_backward_weights(const float* x, const float* dy0, const float* dy1, const float* dy2, int64_t b, int cin, int64_t hw,
                                             int c0, int c1, int c2, float* dw0, float* dw1, float* dw2, float* db0, float* db1, float* db2,
                                             void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  H1 a = {};
  if (int rc = h1_geom("fv2p_head1x1_backward_weights", b, cin, hw, c0, c1, c2, &a)) return rc;
  FV2P_REQUIRE(x && dw0 && dy0 && (!c1 || (dw1 && dy1)) && (!c2 || (dw2 && dy2)), FV2P_EINVAL,
               "fv2p_head1x1_backward_weights: null map, gradient or output");
  FV2P_REQUIRE(ws && ws_bytes >= h1_ws_bytes(a), FV2P_EWORKSPACE, "fv2p_head1x1_backward_weights: workspace of %zu bytes, %zu needed", ws_bytes,
               h1_ws_bytes(a));
  a.x = x;
  a.dy[0] = dy0; a.dy[1] = dy1; a.dy[2] = dy2;
  a.dw[0] = dw0; a.dw[1] = dw1; a.dw[2] = dw2;
  a.db[0] = db0; a.db[1] = db1; a.db[2] = db2;
  Carver cv(ws, ws_bytes);
  a.part = cv.take<double>(static_cast<size_t>(a.splits) * a.np * a.cin + static_cast<size_t>(a.splits) * 4 * 64);
  const bool vec = a.p % 4 == 0 && aligned16(x);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(a.splits), static_cast<unsigned>((cin + 63) / 64));
  H1_DISPATCH(head1x1_bwd_weights_k, a.np / 16, vec, grid, st, a);
  FV2P_LAUNCH_CHECK();
  const dim3 fgrid(static_cast<unsigned>(ceil_div(static_cast<int64_t>(a.tot) * cin + a.tot, 256)));
  hipLaunchKernelGGL(head1x1_fold_k, fgrid, dim3(256), 0, st, a);
  FV2P_LAUNCH_CHECK();
  return 0;
}
