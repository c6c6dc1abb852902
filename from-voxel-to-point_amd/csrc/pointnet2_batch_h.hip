// Batched pointnet2 gather, grouping and interpolation on 16-bit feature rows (float16 / bfloat16).
//
// The 16-bit siblings of fv2p_gather_points, fv2p_group_points_batch and fv2p_three_interpolate_batch (pointnet2.hip; the reference's
// pcdet/ops/pointnet2/pointnet2_batch/src/{sampling,group_points,interpolate}_gpu.cu are float only).  Layouts are the fp32 ops':
// features [B][C][N] channel-major, idx int32, weight fp32.  The contiguous axis of every tensor is the point / sample axis, so the
// 16-byte path of the forward kernels is 8 consecutive OUTPUTS of one (b, c) row: the 8 indices arrive as two 16-byte loads, the 8
// values as two-byte gathers from a feature row that stays in cache (512 points = 1 KB), and leave as one 16-byte store.  A thread keeps
// its indices (and weights) for kChanTile channels, so a sample's index list is read C / kChanTile times instead of C times.
// Gradients: the entries of det_batch_entries_k's order, summed by scatter_add_h into a 16-bit [B * rows][C] staging image, then one
// 16-bit transpose into [B][C][rows] - the route of det_batch_grad (pointnet2.hip) with every row rounded once.
#include "common.hpp"
#include "dt16.hpp"

namespace fv2p {

constexpr int kChanTile = 4;   // channels of the same outputs per thread

// gather / grouping forward: out[b][ch][p] = points[b][ch][idx[b][p]], a copy of bit patterns (one kernel for both formats, and for both
// ops: grouping is the gather with P = npoints * nsample).  thread = (b, tile of kChanTile channels, V consecutive outputs), outputs
// fastest: neighbouring lanes store neighbouring 16-byte pieces of a channel row.  An index outside [0, n) gives zeros.
template <int V>
__global__ __launch_bounds__(256) void gather_rows_h_k(int64_t threads, int c, int n, int64_t P, const u16* __restrict__ points,
                                                        const int* __restrict__ idx, u16* __restrict__ out) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= threads) return;
  const int64_t pv = P / V;
  const int tiles = (c + kChanTile - 1) / kChanTile;
  const int64_t p0 = (t % pv) * V;
  const int ch0 = static_cast<int>((t / pv) % tiles) * kChanTile;
  const int64_t b = t / pv / tiles;
  int id[V];
  if constexpr (V == 8) {
    const int4* ip = reinterpret_cast<const int4*>(idx + b * P + p0);
    const int4 a = ip[0], d = ip[1];
    id[0] = a.x; id[1] = a.y; id[2] = a.z; id[3] = a.w; id[4] = d.x; id[5] = d.y; id[6] = d.z; id[7] = d.w;
  } else {
    id[0] = idx[b * P + p0];
  }
#pragma unroll
  for (int k = 0; k < kChanTile; ++k) {
    const int ch = ch0 + k;
    if (ch >= c) break;
    const u16* row = points + (b * c + ch) * n;
    u16 v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = id[j] >= 0 && id[j] < n ? row[id[j]] : static_cast<u16>(0);
    u16* o = out + (b * c + ch) * P + p0;
    if constexpr (V == 8) {
      unsigned w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = static_cast<unsigned>(v[2 * j]) | (static_cast<unsigned>(v[2 * j + 1]) << 16);
      *reinterpret_cast<uint4*>(o) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      *o = v[0];
    }
  }
}

// interpolation forward: out[b][ch][q] = w0 * f0 + w1 * f1 + w2 * f2 on the widened values, in three_interp_batch_k's order (no
// contraction: the file is built with -ffp-contract=off), rounded once.  thread = (b, channel tile, V consecutive queries): the 3 V
// indices and weights are 16-byte loads of the contiguous [n][3] lists.  A known index outside [0, m) counts as a zero.
template <class T, int V>
__global__ __launch_bounds__(256) void three_interp_batch_h_k(int64_t threads, int c, int m, int n, const u16* __restrict__ points,
                                                               const int* __restrict__ idx, const float* __restrict__ weight,
                                                               u16* __restrict__ out) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= threads) return;
  const int64_t pv = n / V;
  const int tiles = (c + kChanTile - 1) / kChanTile;
  const int64_t q0 = (t % pv) * V;
  const int ch0 = static_cast<int>((t / pv) % tiles) * kChanTile;
  const int64_t b = t / pv / tiles;
  const int64_t e0 = (b * n + q0) * 3;
  int id[3 * V];
  float w[3 * V];
  if constexpr (V == 8) {
    const int4* ip = reinterpret_cast<const int4*>(idx + e0);
    const float4* wp = reinterpret_cast<const float4*>(weight + e0);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int4 a = ip[j];
      const float4 f = wp[j];
      id[4 * j] = a.x; id[4 * j + 1] = a.y; id[4 * j + 2] = a.z; id[4 * j + 3] = a.w;
      w[4 * j] = f.x; w[4 * j + 1] = f.y; w[4 * j + 2] = f.z; w[4 * j + 3] = f.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j) { id[j] = idx[e0 + j]; w[j] = weight[e0 + j]; }
  }
#pragma unroll
  for (int k = 0; k < kChanTile; ++k) {
    const int ch = ch0 + k;
    if (ch >= c) break;
    const u16* row = points + (b * c + ch) * m;
    Row16<T, V> o;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float f[3];
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int r = id[3 * j + s];
        f[s] = r >= 0 && r < m ? T::widen(row[r]) : 0.f;
      }
      o.v[j] = w[3 * j] * f[0] + w[3 * j + 1] * f[1] + w[3 * j + 2] * f[2];
    }
    o.store(out + (b * c + ch) * n + q0);
  }
}

// entries of the batch-layout gradients, as det_batch_entries_k (pointnet2.hip) builds them: grad_out [B][C][P], `per` = div * P entries
// per sample, entry e = (b, j) -> row b * rows + idx[e] of the [B * rows][C] staging image (dropped outside [0, rows)), source column
// j / div of sample b
__global__ void batch_entries_h_k(int64_t entries, int64_t per, int div, int c, int rows, const int* __restrict__ idx, int* __restrict__ dst,
                                  int64_t* __restrict__ off) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= entries) return;
  const int64_t b = e / per, j = e % per;
  const int i = idx[e];
  dst[e] = i >= 0 && i < rows ? static_cast<int>(b * rows + i) : -1;
  off[e] = b * c * (per / div) + j / div;
}

}  // namespace fv2p
using namespace fv2p;

#define G1D(total) dim3(static_cast<unsigned>(ceil_div((total), 256))), dim3(256)
#define STREAM(s) static_cast<hipStream_t>(s)
#define FV2P_DT16_OK(who, dtype) FV2P_REQUIRE((dtype) == FV2P_DT_F16 || (dtype) == FV2P_DT_BF16, FV2P_EINVAL, "%s: dtype %d is neither fp16 (1) nor bf16 (2)", who, (dtype))

static int64_t chan_tiles(int c) { return (static_cast<int64_t>(c) + kChanTile - 1) / kChanTile; }

// out [B][C][P] = points [B][C][n] at idx [B][P]
static int gather_rows_h(const char* who, int b, int c, int n, int64_t P, const void* points, const int* idx, void* out, int dtype, hipStream_t st) {
  FV2P_DT16_OK(who, dtype);
  FV2P_REQUIRE(b >= 0 && c >= 1 && n >= 0 && P >= 0, FV2P_EINVAL, "%s: bad sizes", who);
  if (b == 0 || P == 0) return 0;
  FV2P_REQUIRE((points || n == 0) && idx && out, FV2P_EINVAL, "%s: null pointer", who);
  const bool vec = P % 8 == 0 && aligned16(idx) && aligned16(out);
  const int64_t threads = static_cast<int64_t>(b) * chan_tiles(c) * (vec ? P / 8 : P);
  FV2P_REQUIRE(ceil_div(threads, 256) < (1ll << 31), FV2P_ELIMIT, "%s: too many elements", who);
  if (vec) hipLaunchKernelGGL((gather_rows_h_k<8>), G1D(threads), 0, st, threads, c, n, P, static_cast<const u16*>(points), idx, static_cast<u16*>(out));
  else hipLaunchKernelGGL((gather_rows_h_k<1>), G1D(threads), 0, st, threads, c, n, P, static_cast<const u16*>(points), idx, static_cast<u16*>(out));
  FV2P_LAUNCH_CHECK();
  return 0;
}

// the lists of det_batch_grad and a 16-bit [B * rows][C] staging image (counted in floats: two elements each), never an fp32 image
static size_t batch_h_stage_floats(int b, int c, int rows) {
  return (static_cast<size_t>(b > 0 ? b : 1) * (rows > 0 ? rows : 1) * (c > 0 ? c : 1) + 1) / 2;
}
static size_t batch_grad_h_ws(int b, int c, int rows, int64_t per) {
  const int64_t entries = static_cast<int64_t>(b > 0 ? b : 0) * (per > 0 ? per : 0);
  return det_lists_bytes(entries, c > 0 ? c : 1, false, batch_h_stage_floats(b, c, rows));
}
// grad_points [B][C][rows] (written) from grad_out [B][C][per / div], entries (b, j) -> row idx[b * per + j], coefficient weight[e] or 1
static int batch_grad_h(const char* who, int b, int c, int rows, int64_t per, int div, const void* grad_out, const int* idx, const float* weight,
                        void* grad_points, int dtype, void* ws, size_t ws_bytes, hipStream_t st) {
  FV2P_DT16_OK(who, dtype);
  FV2P_REQUIRE(b >= 0 && c >= 1 && rows >= 0 && per >= 0, FV2P_EINVAL, "%s: bad sizes", who);
  const int64_t out_n = static_cast<int64_t>(b) * c * rows;
  if (out_n == 0) return 0;
  FV2P_REQUIRE(grad_points, FV2P_EINVAL, "%s: null pointer", who);
  const int64_t entries = static_cast<int64_t>(b) * per;
  FV2P_REQUIRE(entries == 0 || (grad_out && idx && (div == 1 || weight)), FV2P_EINVAL, "%s: null pointer", who);
  FV2P_REQUIRE(entries < (1ll << 31) && static_cast<int64_t>(b) * rows < (1ll << 30), FV2P_ELIMIT, "%s: too many entries", who);
  if (entries == 0) { FV2P_HIP(hipMemsetAsync(grad_points, 0, static_cast<size_t>(out_n) * sizeof(u16), st)); return 0; }
  FV2P_REQUIRE(ws && ws_bytes >= batch_grad_h_ws(b, c, rows, per), FV2P_EWORKSPACE, "%s: workspace too small", who);
  const DetLists d = det_lists(ws, ws_bytes, entries, c, false, batch_h_stage_floats(b, c, rows));
  u16* stage = reinterpret_cast<u16*>(d.stage);
  hipLaunchKernelGGL(batch_entries_h_k, G1D(entries), 0, st, entries, per, div, c, rows, idx, d.dst, d.off);
  if (int rc = scatter_add_h(entries, c, static_cast<int64_t>(b) * rows, d.dst, d.off, weight, grad_out, per / div, stage, dtype, d.sws,
                             d.sws_bytes, st)) return rc;   // zero-fills the staging image
  return fv2p_transpose_batched_h(stage, b, rows, c, grad_points, st);   // [B][rows][C] -> [B][C][rows]
}

extern "C" int fv2p_gather_points_h(int b, int c, int n, int npoints, const void* points, const int* idx, void* out, int dtype, fv2p_stream_t s) {
  FV2P_REQUIRE(npoints >= 0, FV2P_EINVAL, "gather_points_h: bad sizes");
  return gather_rows_h("gather_points_h", b, c, n, npoints, points, idx, out, dtype, STREAM(s));
}
extern "C" size_t fv2p_gather_points_grad_h_ws_bytes(int b, int c, int n, int npoints) { return batch_grad_h_ws(b, c, n, npoints); }
extern "C" int fv2p_gather_points_grad_h(int b, int c, int n, int npoints, const void* grad_out, const int* idx, void* grad_points, int dtype,
                                         void* ws, size_t ws_bytes, fv2p_stream_t s) {
  return batch_grad_h("gather_points_grad_h", b, c, n, npoints, 1, grad_out, idx, nullptr, grad_points, dtype, ws, ws_bytes, STREAM(s));
}

extern "C" int fv2p_group_points_batch_h(int b, int c, int n, int npoints, int nsample, const void* points, const int* idx, void* out, int dtype,
                                         fv2p_stream_t s) {
  FV2P_REQUIRE(npoints >= 0 && nsample >= 0, FV2P_EINVAL, "group_points_batch_h: bad sizes");
  return gather_rows_h("group_points_batch_h", b, c, n, static_cast<int64_t>(npoints) * nsample, points, idx, out, dtype, STREAM(s));
}
extern "C" size_t fv2p_group_points_batch_grad_h_ws_bytes(int b, int c, int n, int npoints, int nsample) {
  return batch_grad_h_ws(b, c, n, static_cast<int64_t>(npoints > 0 ? npoints : 0) * (nsample > 0 ? nsample : 0));
}
extern "C" int fv2p_group_points_batch_grad_h(int b, int c, int n, int npoints, int nsample, const void* grad_out, const int* idx, void* grad_points,
                                              int dtype, void* ws, size_t ws_bytes, fv2p_stream_t s) {
  FV2P_REQUIRE(npoints >= 0 && nsample >= 0, FV2P_EINVAL, "group_points_batch_grad_h: bad sizes");
  return batch_grad_h("group_points_batch_grad_h", b, c, n, static_cast<int64_t>(npoints) * nsample, 1, grad_out, idx, nullptr, grad_points, dtype,
                      ws, ws_bytes, STREAM(s));
}

template <class T>
static void launch_interp_batch_h(bool vec, int64_t threads, int c, int m, int n, const void* points, const int* idx, const float* weight, void* out,
                                  hipStream_t st) {
  if (vec) hipLaunchKernelGGL((three_interp_batch_h_k<T, 8>), G1D(threads), 0, st, threads, c, m, n, static_cast<const u16*>(points), idx, weight,
                              static_cast<u16*>(out));
  else hipLaunchKernelGGL((three_interp_batch_h_k<T, 1>), G1D(threads), 0, st, threads, c, m, n, static_cast<const u16*>(points), idx, weight,
                          static_cast<u16*>(out));
}
extern "C" int fv2p_three_interpolate_batch_h(int b, int c, int m, int n, const void* points, const int* idx, const float* weight, void* out, int dtype,
                                              fv2p_stream_t s) {
  FV2P_DT16_OK("three_interpolate_batch_h", dtype);
  FV2P_REQUIRE(b >= 0 && c >= 1 && m >= 0 && n >= 0, FV2P_EINVAL, "three_interpolate_batch_h: bad sizes");
  if (b == 0 || n == 0) return 0;
  FV2P_REQUIRE((points || m == 0) && idx && weight && out, FV2P_EINVAL, "three_interpolate_batch_h: null pointer");
  const bool vec = n % 8 == 0 && aligned16(idx) && aligned16(weight) && aligned16(out);
  const int64_t threads = static_cast<int64_t>(b) * chan_tiles(c) * (vec ? n / 8 : n);
  FV2P_REQUIRE(ceil_div(threads, 256) < (1ll << 31), FV2P_ELIMIT, "three_interpolate_batch_h: too many elements");
  if (dtype == FV2P_DT_F16) launch_interp_batch_h<H16>(vec, threads, c, m, n, points, idx, weight, out, STREAM(s));
  else launch_interp_batch_h<B16>(vec, threads, c, m, n, points, idx, weight, out, STREAM(s));
  FV2P_LAUNCH_CHECK();
  return 0;
}
extern "C" size_t fv2p_three_interpolate_batch_grad_h_ws_bytes(int b, int c, int n, int m) {
  return batch_grad_h_ws(b, c, m, static_cast<int64_t>(n > 0 ? n : 0) * 3);
}
// grad_out (B,C,n), idx / weight (B,n,3) -> grad_points (B,C,m): entry e = 3 * (b * n + query) + slot, coefficient weight[e]
extern "C" int fv2p_three_interpolate_batch_grad_h(int b, int c, int n, int m, const void* grad_out, const int* idx, const float* weight,
                                                   void* grad_points, int dtype, void* ws, size_t ws_bytes, fv2p_stream_t s) {
  FV2P_REQUIRE(n >= 0, FV2P_EINVAL, "three_interpolate_batch_grad_h: bad sizes");
  return batch_grad_h("three_interpolate_batch_grad_h", b, c, m, static_cast<int64_t>(n) * 3, 3, grad_out, idx, weight, grad_points, dtype, ws,
                      ws_bytes, STREAM(s));
}
