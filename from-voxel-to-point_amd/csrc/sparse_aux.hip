// A7 — sparse max-pool and neighbour "group" over the rulebook tables.
// Replaces indice_maxpool_{fp32,half}(+backward) (pcdet/ops/spconv/include/spconv/pool_ops.h:25-94,
// src/maxpool_cuda.cu:28-454) and indice_group_fp32(+backward) (include/spconv/group_ops.h:29-291).
// Both are pure gathers once the rulebook is a table: one thread per (row, channel quad), no atomics.
#include "common.hpp"
#include "dt16.hpp"

namespace fv2p {

// out[o,c] = max(0, max_k in[tab[k][o], c])  — the reference starts from a zero-filled output and only
// overwrites when in > out (pool_ops.h:34, maxpool_cuda.cu:47-49), so negatives clamp to 0.
__global__ void maxpool_fwd(const float* __restrict__ in, int c, const int* __restrict__ tab, int kvol, int n_out, int flip,
                            float* __restrict__ out) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= static_cast<int64_t>(n_out) * c) return;
  const int o = static_cast<int>(t / c), ch = static_cast<int>(t % c);
  float m = 0.f;
  for (int k = 0; k < kvol; ++k) {
    const int i = tab[static_cast<int64_t>(flip ? kvol - 1 - k : k) * n_out + o];
    if (i >= 0) {
      const float v = in[static_cast<int64_t>(i) * c + ch];
      if (v > m) m = v;
    }
  }
  out[t] = m;
}

// din[i,c] = sum_k [in[i,c] == out[tab_in[k][i], c]] * dout[tab_in[k][i], c]   (maxpool_cuda.cu:188-190)
__global__ void maxpool_bwd(const float* __restrict__ in, const float* __restrict__ out, const float* __restrict__ dout, int n_in,
                            int c, const int* __restrict__ tab_in, int kvol, float* __restrict__ din) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= static_cast<int64_t>(n_in) * c) return;
  const int i = static_cast<int>(t / c), ch = static_cast<int>(t % c);
  const float v = in[t];
  float g = 0.f;
  for (int k = 0; k < kvol; ++k) {
    const int o = tab_in[static_cast<int64_t>(k) * n_in + i];
    if (o >= 0 && out[static_cast<int64_t>(o) * c + ch] == v) g += dout[static_cast<int64_t>(o) * c + ch];
  }
  din[t] = g;
}

// The same two on 16-bit rows (float16 / bfloat16): one thread per (row, V channels), V = 8 as one 16-byte access when c % 8 == 0.
// Compared on the widened values; the forward result is one of its inputs or 0 (exact), the backward sum runs in fp32 over
// ascending k and is rounded once.
template <class T, int V>
__global__ __launch_bounds__(256) void maxpool_fwd_h(const u16* __restrict__ in, int c, const int* __restrict__ tab, int kvol, int n_out, int flip,
                                                     u16* __restrict__ out) {
  const int cv = c / V;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= static_cast<int64_t>(n_out) * cv) return;
  const int o = static_cast<int>(t / cv), ch = static_cast<int>(t % cv) * V;
  Row16<T, V> m;
#pragma unroll
  for (int j = 0; j < V; ++j) m.v[j] = 0.f;
  for (int k = 0; k < kvol; ++k) {
    const int i = tab[static_cast<int64_t>(flip ? kvol - 1 - k : k) * n_out + o];
    if (i >= 0) {
      Row16<T, V> v;
      v.load(in + static_cast<int64_t>(i) * c + ch);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (v.v[j] > m.v[j]) m.v[j] = v.v[j];
    }
  }
  m.store(out + static_cast<int64_t>(o) * c + ch);
}

template <class T, int V>
__global__ __launch_bounds__(256) void maxpool_bwd_h(const u16* __restrict__ in, const u16* __restrict__ out, const u16* __restrict__ dout, int n_in,
                                                     int c, const int* __restrict__ tab_in, int kvol, u16* __restrict__ din) {
  const int cv = c / V;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= static_cast<int64_t>(n_in) * cv) return;
  const int i = static_cast<int>(t / cv), ch = static_cast<int>(t % cv) * V;
  Row16<T, V> v, g;
  v.load(in + static_cast<int64_t>(i) * c + ch);
#pragma unroll
  for (int j = 0; j < V; ++j) g.v[j] = 0.f;
  for (int k = 0; k < kvol; ++k) {
    const int o = tab_in[static_cast<int64_t>(k) * n_in + i];
    if (o >= 0) {
      Row16<T, V> ov, dv;
      ov.load(out + static_cast<int64_t>(o) * c + ch);
      dv.load(dout + static_cast<int64_t>(o) * c + ch);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (ov.v[j] == v.v[j]) g.v[j] += dv.v[j];
    }
  }
  g.store(din + static_cast<int64_t>(i) * c + ch);
}

// out[k, o, :] = in[tab[k][o], :] or 0
__global__ void group_fwd(const float* __restrict__ in, int c, const int* __restrict__ tab, int kvol, int n_out, int flip,
                          float* __restrict__ out) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t per_k = static_cast<int64_t>(n_out) * c;
  if (t >= per_k * kvol) return;
  const int k = static_cast<int>(t / per_k);
  const int64_t r = t % per_k;
  const int o = static_cast<int>(r / c), ch = static_cast<int>(r % c);
  const int i = tab[static_cast<int64_t>(flip ? kvol - 1 - k : k) * n_out + o];
  out[t] = i >= 0 ? in[static_cast<int64_t>(i) * c + ch] : 0.f;
}

// din[i,:] = sum_k g[k, tab[k][i], :]
__global__ void group_bwd(const float* __restrict__ g, int n_out, int c, const int* __restrict__ tab, int kvol, int n_in, int flip,
                          float* __restrict__ din) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= static_cast<int64_t>(n_in) * c) return;
  const int i = static_cast<int>(t / c), ch = static_cast<int>(t % c);
  float s = 0.f;
  for (int k = 0; k < kvol; ++k) {
    const int o = tab[static_cast<int64_t>(flip ? kvol - 1 - k : k) * n_in + i];
    if (o >= 0) s += g[(static_cast<int64_t>(k) * n_out + o) * c + ch];
  }
  din[t] = s;
}

// The group pair on 16-bit rows.  The forward is a copy (no value is looked at: one kernel for both formats), V = 8 channels as one
// 16-byte access when c % 8 == 0; the backward widens, sums in fp32 over ascending k and rounds once.
template <int V>
__global__ __launch_bounds__(256) void group_fwd_h(const u16* __restrict__ in, int c, const int* __restrict__ tab, int kvol, int n_out, int flip,
                                                   u16* __restrict__ out) {
  const int cv = c / V;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t per_k = static_cast<int64_t>(n_out) * cv;
  if (t >= per_k * kvol) return;
  const int k = static_cast<int>(t / per_k);
  const int64_t r = t % per_k;
  const int o = static_cast<int>(r / cv), ch = static_cast<int>(r % cv) * V;
  const int i = tab[static_cast<int64_t>(flip ? kvol - 1 - k : k) * n_out + o];
  u16* dst = out + (static_cast<int64_t>(k) * n_out + o) * c + ch;
  if constexpr (V == 8) *reinterpret_cast<uint4*>(dst) = i >= 0 ? *reinterpret_cast<const uint4*>(in + static_cast<int64_t>(i) * c + ch) : make_uint4(0, 0, 0, 0);
  else *dst = i >= 0 ? in[static_cast<int64_t>(i) * c + ch] : static_cast<u16>(0);
}
template <class T, int V>
__global__ __launch_bounds__(256) void group_bwd_h(const u16* __restrict__ g, int n_out, int c, const int* __restrict__ tab, int kvol, int n_in, int flip,
                                                   u16* __restrict__ din) {
  const int cv = c / V;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= static_cast<int64_t>(n_in) * cv) return;
  const int i = static_cast<int>(t / cv), ch = static_cast<int>(t % cv) * V;
  Row16<T, V> s;
#pragma unroll
  for (int j = 0; j < V; ++j) s.v[j] = 0.f;
  for (int k = 0; k < kvol; ++k) {
    const int o = tab[static_cast<int64_t>(flip ? kvol - 1 - k : k) * n_in + i];
    if (o >= 0 && o < n_out) {
      Row16<T, V> v;
      v.load(g + (static_cast<int64_t>(k) * n_out + o) * c + ch);
#pragma unroll
      for (int j = 0; j < V; ++j) s.v[j] += v.v[j];
    }
  }
  s.store(din + static_cast<int64_t>(i) * c + ch);
}

// ---- SparseConvTensor.dense() --------------------------------------------------------------------
// The reference builds the dense tensor as zeros [B, *spatial, C] -> index scatter -> permute(0, C, ...).contiguous()
// (structure.py:57-66, used by HeightCompression, height_compression.py:10-26): three passes over the dense volume.
// Here: one fill + one scatter straight into the requested layout.  vol = D*H*W cells per sample.
//   channels_first: out[b][ch][cell]   (thread = (ch, row): rows sorted by cell -> neighbouring threads write neighbouring x)
//   channels_last : out[b][cell][ch]   (thread = (row, ch): whole rows contiguous)
__global__ __launch_bounds__(256) void dense_scatter(const float* __restrict__ feat, const int* __restrict__ ind, int n, int c, int ndim,
                                                     int d1, int d2, int64_t vol, int channels_first, float* __restrict__ out) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= static_cast<int64_t>(n) * c) return;
  const int row = channels_first ? static_cast<int>(t % n) : static_cast<int>(t / c);
  const int ch = channels_first ? static_cast<int>(t / n) : static_cast<int>(t % c);
  const int* p = ind + static_cast<int64_t>(row) * (ndim + 1);
  const int64_t cell = ndim == 3 ? (static_cast<int64_t>(p[1]) * d1 + p[2]) * d2 + p[3] : static_cast<int64_t>(p[1]) * d2 + p[2];
  const int64_t b = p[0];
  const float v = feat[static_cast<int64_t>(row) * c + ch];
  if (channels_first) out[(b * c + ch) * vol + cell] = v;
  else out[(b * vol + cell) * c + ch] = v;
}
// gradient of dense(): drows[row][ch] = ddense at the row's cell
__global__ __launch_bounds__(256) void dense_gather(const float* __restrict__ dense, const int* __restrict__ ind, int n, int c, int ndim,
                                                    int d1, int d2, int64_t vol, int channels_first, float* __restrict__ rows) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= static_cast<int64_t>(n) * c) return;
  const int row = channels_first ? static_cast<int>(t % n) : static_cast<int>(t / c);
  const int ch = channels_first ? static_cast<int>(t / n) : static_cast<int>(t % c);
  const int* p = ind + static_cast<int64_t>(row) * (ndim + 1);
  const int64_t cell = ndim == 3 ? (static_cast<int64_t>(p[1]) * d1 + p[2]) * d2 + p[3] : static_cast<int64_t>(p[1]) * d2 + p[2];
  const int64_t b = p[0];
  rows[static_cast<int64_t>(row) * c + ch] = channels_first ? dense[(b * c + ch) * vol + cell] : dense[(b * vol + cell) * c + ch];
}

// dense() and its gradient on 16-bit rows: copies, so one kernel serves float16 and bfloat16.
//   channels_last, V = 8: thread = (row, 8 channels), one 16-byte load and one 16-byte store (c % 8 == 0, both bases 16-byte aligned)
//   channels_last, V = 1: thread = (row, ch)
//   channels_first      : thread = (ch, row) as in dense_scatter: rows sorted by cell -> neighbouring lanes hit neighbouring cells
template <int V, bool kGather>
__global__ __launch_bounds__(256) void dense_move_h(const int* __restrict__ ind, int n, int c, int ndim, int d1, int d2, int64_t vol, int channels_first,
                                                    u16* __restrict__ rows, u16* __restrict__ dense) {
  const int cv = c / V;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= static_cast<int64_t>(n) * cv) return;
  const int row = channels_first ? static_cast<int>(t % n) : static_cast<int>(t / cv);
  const int ch = (channels_first ? static_cast<int>(t / n) : static_cast<int>(t % cv)) * V;
  const int* p = ind + static_cast<int64_t>(row) * (ndim + 1);
  const int64_t cell = ndim == 3 ? (static_cast<int64_t>(p[1]) * d1 + p[2]) * d2 + p[3] : static_cast<int64_t>(p[1]) * d2 + p[2];
  const int64_t b = p[0];
  u16* r = rows + static_cast<int64_t>(row) * c + ch;
  u16* d = dense + (channels_first ? (b * c + ch) * vol + cell : (b * vol + cell) * c + ch);
  if constexpr (V == 8) {
    if (kGather) *reinterpret_cast<uint4*>(r) = *reinterpret_cast<const uint4*>(d);
    else *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(r);
  } else {
    if (kGather) *r = *d;
    else *d = *r;
  }
}

// ---- MeanVFE + collate of one voxelised cloud -------------------------------------------------------
// mean over the first num_points[v] points of voxel v (pcdet/models/backbones_3d/vfe/mean_vfe.py:14-31: sum over the
// zero-padded slots / clamp_min(num, 1)) and (batch_idx, z, y, x) coordinates (dataset.collate_batch,
// pcdet/datasets/dataset.py:165-171), written at this cloud's offset of the batch tensors; the voxel count is read on
// the device, so the launch needs no host round trip of its own.
__global__ __launch_bounds__(256) void voxel_mean_collate(const float* __restrict__ voxels, const int* __restrict__ coors,
                                                          const int* __restrict__ num, const int* __restrict__ count, int max_voxels,
                                                          int max_pts, int ndim, int batch_idx, float* __restrict__ feats,
                                                          int* __restrict__ coords) {
  const int m = min(*count, max_voxels);
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= static_cast<int64_t>(m) * ndim) return;
  const int v = static_cast<int>(t / ndim), d = static_cast<int>(t % ndim);
  float s = 0.f;
  for (int p = 0; p < max_pts; ++p) s += voxels[(static_cast<int64_t>(v) * max_pts + p) * ndim + d];
  const int k = num[v];
  feats[static_cast<int64_t>(v) * ndim + d] = s / static_cast<float>(k < 1 ? 1 : k);
  if (d < 4) coords[static_cast<int64_t>(v) * 4 + d] = d == 0 ? batch_idx : coors[static_cast<int64_t>(v) * 3 + d - 1];
}

}  // namespace fv2p
using namespace fv2p;

#define FV2P_GRID1D(total) dim3(static_cast<unsigned>(ceil_div((total), 256))), dim3(256)

extern "C" int fv2p_sparse_maxpool_fwd(const float* in, int64_t n_in, int c, const int* tab, int kvol, int64_t n_out, int flip_k,
                                       float* out, fv2p_stream_t s) {
  FV2P_REQUIRE(c >= 1 && kvol >= 1 && n_out >= 0, FV2P_EINVAL, "maxpool_fwd: bad sizes");
  if (n_out == 0) return 0;
  FV2P_REQUIRE(in && tab && out, FV2P_EINVAL, "maxpool_fwd: null pointer");
  hipLaunchKernelGGL(maxpool_fwd, FV2P_GRID1D(n_out * c), 0, static_cast<hipStream_t>(s), in, c, tab, kvol, (int)n_out, flip_k & 1, out);
  FV2P_LAUNCH_CHECK();
  return 0;
}
extern "C" int fv2p_sparse_maxpool_bwd(const float* in, const float* out, const float* dout, int64_t n_in, int c, const int* tab_in,
                                       int kvol, float* din, fv2p_stream_t s) {
  FV2P_REQUIRE(c >= 1 && kvol >= 1 && n_in >= 0, FV2P_EINVAL, "maxpool_bwd: bad sizes");
  if (n_in == 0) return 0;
  FV2P_REQUIRE(in && out && dout && tab_in && din, FV2P_EINVAL, "maxpool_bwd: null pointer");
  hipLaunchKernelGGL(maxpool_bwd, FV2P_GRID1D(n_in * c), 0, static_cast<hipStream_t>(s), in, out, dout, (int)n_in, c, tab_in, kvol, din);
  FV2P_LAUNCH_CHECK();
  return 0;
}
template <class T>
static void launch_maxpool_fwd_h(bool vec, const void* in, int c, const int* tab, int kvol, int64_t n_out, int flip, void* out, hipStream_t s) {
  if (vec) hipLaunchKernelGGL((maxpool_fwd_h<T, 8>), FV2P_GRID1D(n_out * (c / 8)), 0, s, static_cast<const u16*>(in), c, tab, kvol, (int)n_out, flip, static_cast<u16*>(out));
  else hipLaunchKernelGGL((maxpool_fwd_h<T, 1>), FV2P_GRID1D(n_out * c), 0, s, static_cast<const u16*>(in), c, tab, kvol, (int)n_out, flip, static_cast<u16*>(out));
}
template <class T>
static void launch_maxpool_bwd_h(bool vec, const void* in, const void* out, const void* dout, int64_t n_in, int c, const int* tab_in, int kvol, void* din,
                                 hipStream_t s) {
  if (vec) hipLaunchKernelGGL((maxpool_bwd_h<T, 8>), FV2P_GRID1D(n_in * (c / 8)), 0, s, static_cast<const u16*>(in), static_cast<const u16*>(out),
                              static_cast<const u16*>(dout), (int)n_in, c, tab_in, kvol, static_cast<u16*>(din));
  else hipLaunchKernelGGL((maxpool_bwd_h<T, 1>), FV2P_GRID1D(n_in * c), 0, s, static_cast<const u16*>(in), static_cast<const u16*>(out),
                          static_cast<const u16*>(dout), (int)n_in, c, tab_in, kvol, static_cast<u16*>(din));
}
extern "C" int fv2p_sparse_maxpool_fwd_h(const void* in, int64_t n_in, int c, const int* tab, int kvol, int64_t n_out, int flip_k, void* out, int dtype,
                                         fv2p_stream_t s) {
  FV2P_DT16_OK("maxpool_fwd_h", dtype);
  FV2P_REQUIRE(c >= 1 && kvol >= 1 && n_out >= 0 && n_in >= 0, FV2P_EINVAL, "maxpool_fwd_h: bad sizes");
  if (n_out == 0) return 0;
  FV2P_REQUIRE(in && tab && out, FV2P_EINVAL, "maxpool_fwd_h: null pointer");
  const bool vec = (c % 8 == 0) && aligned16(in) && aligned16(out);
  if (dtype == FV2P_DT_F16) launch_maxpool_fwd_h<H16>(vec, in, c, tab, kvol, n_out, flip_k & 1, out, static_cast<hipStream_t>(s));
  else launch_maxpool_fwd_h<B16>(vec, in, c, tab, kvol, n_out, flip_k & 1, out, static_cast<hipStream_t>(s));
  FV2P_LAUNCH_CHECK();
  return 0;
}
extern "C" int fv2p_sparse_maxpool_bwd_h(const void* in, const void* out, const void* dout, int64_t n_in, int c, const int* tab_in, int kvol, void* din,
                                         int dtype, fv2p_stream_t s) {
  FV2P_DT16_OK("maxpool_bwd_h", dtype);
  FV2P_REQUIRE(c >= 1 && kvol >= 1 && n_in >= 0, FV2P_EINVAL, "maxpool_bwd_h: bad sizes");
  if (n_in == 0) return 0;
  FV2P_REQUIRE(in && out && dout && tab_in && din, FV2P_EINVAL, "maxpool_bwd_h: null pointer");
  const bool vec = (c % 8 == 0) && aligned16(in) && aligned16(out) && aligned16(dout) && aligned16(din);
  if (dtype == FV2P_DT_F16) launch_maxpool_bwd_h<H16>(vec, in, out, dout, n_in, c, tab_in, kvol, din, static_cast<hipStream_t>(s));
  else launch_maxpool_bwd_h<B16>(vec, in, out, dout, n_in, c, tab_in, kvol, din, static_cast<hipStream_t>(s));
  FV2P_LAUNCH_CHECK();
  return 0;
}
extern "C" int fv2p_sparse_group_fwd(const float* in, int64_t n_in, int c, const int* tab, int kvol, int64_t n_out, int flip_k,
                                     float* out, fv2p_stream_t s) {
  FV2P_REQUIRE(c >= 1 && kvol >= 1 && n_out >= 0, FV2P_EINVAL, "group_fwd: bad sizes");
  if (n_out == 0) return 0;
  FV2P_REQUIRE(in && tab && out, FV2P_EINVAL, "group_fwd: null pointer");
  hipLaunchKernelGGL(group_fwd, FV2P_GRID1D(n_out * c * kvol), 0, static_cast<hipStream_t>(s), in, c, tab, kvol, (int)n_out, flip_k & 1, out);
  FV2P_LAUNCH_CHECK();
  return 0;
}
extern "C" int fv2p_sparse_group_bwd(const float* grad, int64_t n_out, int c, const int* tab, int kvol, int64_t n_in, int flip_k,
                                     float* din, fv2p_stream_t s) {
  FV2P_REQUIRE(c >= 1 && kvol >= 1 && n_in >= 0, FV2P_EINVAL, "group_bwd: bad sizes");
  if (n_in == 0) return 0;
  FV2P_REQUIRE(grad && tab && din, FV2P_EINVAL, "group_bwd: null pointer");
  hipLaunchKernelGGL(group_bwd, FV2P_GRID1D(n_in * c), 0, static_cast<hipStream_t>(s), grad, (int)n_out, c, tab, kvol, (int)n_in, flip_k & 1, din);
  FV2P_LAUNCH_CHECK();
  return 0;
}

template <class T>
static void launch_group_bwd_h(bool vec, const void* g, int64_t n_out, int c, const int* tab, int kvol, int64_t n_in, int flip, void* din, hipStream_t s) {
  if (vec) hipLaunchKernelGGL((group_bwd_h<T, 8>), FV2P_GRID1D(n_in * (c / 8)), 0, s, static_cast<const u16*>(g), (int)n_out, c, tab, kvol, (int)n_in, flip, static_cast<u16*>(din));
  else hipLaunchKernelGGL((group_bwd_h<T, 1>), FV2P_GRID1D(n_in * c), 0, s, static_cast<const u16*>(g), (int)n_out, c, tab, kvol, (int)n_in, flip, static_cast<u16*>(din));
}
extern "C" int fv2p_sparse_group_fwd_h(const void* in, int64_t n_in, int c, const int* tab, int kvol, int64_t n_out, int flip_k, void* out, int dtype,
                                       fv2p_stream_t s) {
  FV2P_DT16_OK("group_fwd_h", dtype);
  FV2P_REQUIRE(c >= 1 && kvol >= 1 && n_out >= 0 && n_in >= 0, FV2P_EINVAL, "group_fwd_h: bad sizes");
  FV2P_REQUIRE(n_out * kvol * c < (1ll << 40) && n_out < (1ll << 31) && n_in < (1ll << 31), FV2P_ELIMIT, "group_fwd_h: too many rows");
  if (n_out == 0) return 0;
  FV2P_REQUIRE(tab && out && (in || n_in == 0), FV2P_EINVAL, "group_fwd_h: null pointer");
  if ((c % 8 == 0) && aligned16(in) && aligned16(out))
    hipLaunchKernelGGL((group_fwd_h<8>), FV2P_GRID1D(n_out * (c / 8) * kvol), 0, static_cast<hipStream_t>(s), static_cast<const u16*>(in), c, tab, kvol, (int)n_out,
                       flip_k & 1, static_cast<u16*>(out));
  else
    hipLaunchKernelGGL((group_fwd_h<1>), FV2P_GRID1D(n_out * c * kvol), 0, static_cast<hipStream_t>(s), static_cast<const u16*>(in), c, tab, kvol, (int)n_out,
                       flip_k & 1, static_cast<u16*>(out));
  FV2P_LAUNCH_CHECK();
  return 0;
}
extern "C" int fv2p_sparse_group_bwd_h(const void* grad, int64_t n_out, int c, const int* tab, int kvol, int64_t n_in, int flip_k, void* din, int dtype,
                                       fv2p_stream_t s) {
  FV2P_DT16_OK("group_bwd_h", dtype);
  FV2P_REQUIRE(c >= 1 && kvol >= 1 && n_in >= 0 && n_out >= 0, FV2P_EINVAL, "group_bwd_h: bad sizes");
  FV2P_REQUIRE(n_out < (1ll << 31) && n_in < (1ll << 31), FV2P_ELIMIT, "group_bwd_h: too many rows");
  if (n_in == 0) return 0;
  FV2P_REQUIRE(tab && din && (grad || n_out == 0), FV2P_EINVAL, "group_bwd_h: null pointer");
  const bool vec = (c % 8 == 0) && aligned16(grad) && aligned16(din);
  if (dtype == FV2P_DT_F16) launch_group_bwd_h<H16>(vec, grad, n_out, c, tab, kvol, n_in, flip_k & 1, din, static_cast<hipStream_t>(s));
  else launch_group_bwd_h<B16>(vec, grad, n_out, c, tab, kvol, n_in, flip_k & 1, din, static_cast<hipStream_t>(s));
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" int fv2p_sparse_to_dense(const float* features, const int* indices, int64_t n, int c, int ndim, int batch,
                                    const int spatial[3], int channels_first, float* dense, fv2p_stream_t s_) {
  hipStream_t s = static_cast<hipStream_t>(s_);
  FV2P_REQUIRE(c >= 1 && n >= 0 && batch >= 1 && (ndim == 2 || ndim == 3), FV2P_EINVAL, "sparse_to_dense: bad sizes");
  FV2P_REQUIRE(dense && spatial, FV2P_EINVAL, "sparse_to_dense: null pointer");
  const int64_t vol = ndim == 3 ? static_cast<int64_t>(spatial[0]) * spatial[1] * spatial[2] : static_cast<int64_t>(spatial[0]) * spatial[1];
  FillJobs fill;
  fill.add(dense, sizeof(float) * static_cast<size_t>(batch) * c * vol, 0u);
  if (int rc = multi_fill(fill, s)) return rc;
  if (n == 0) return 0;
  FV2P_REQUIRE(features && indices, FV2P_EINVAL, "sparse_to_dense: null pointer");
  hipLaunchKernelGGL(dense_scatter, FV2P_GRID1D(n * c), 0, s, features, indices, (int)n, c, ndim, ndim == 3 ? spatial[1] : 0,
                     ndim == 3 ? spatial[2] : spatial[1], vol, channels_first, dense);
  FV2P_LAUNCH_CHECK();
  return 0;
}
extern "C" int fv2p_dense_to_sparse(const float* dense, const int* indices, int64_t n, int c, int ndim, int batch, const int spatial[3],
                                    int channels_first, float* rows, fv2p_stream_t s_) {
  hipStream_t s = static_cast<hipStream_t>(s_);
  FV2P_REQUIRE(c >= 1 && n >= 0 && batch >= 1 && (ndim == 2 || ndim == 3), FV2P_EINVAL, "dense_to_sparse: bad sizes");
  if (n == 0) return 0;
  FV2P_REQUIRE(dense && indices && rows && spatial, FV2P_EINVAL, "dense_to_sparse: null pointer");
  const int64_t vol = ndim == 3 ? static_cast<int64_t>(spatial[0]) * spatial[1] * spatial[2] : static_cast<int64_t>(spatial[0]) * spatial[1];
  hipLaunchKernelGGL(dense_gather, FV2P_GRID1D(n * c), 0, s, dense, indices, (int)n, c, ndim, ndim == 3 ? spatial[1] : 0,
                     ndim == 3 ? spatial[2] : spatial[1], vol, channels_first, rows);
  FV2P_LAUNCH_CHECK();
  return 0;
}
// the 16-bit pair: the same arguments plus dtype; the values are moved, never looked at
template <bool kGather>
static void launch_dense_move_h(const int* ind, int64_t n, int c, int ndim, const int spatial[3], int64_t vol, int channels_first, void* rows, void* dense,
                                hipStream_t s) {
  const int d1 = ndim == 3 ? spatial[1] : 0, d2 = ndim == 3 ? spatial[2] : spatial[1];
  if (!channels_first && c % 8 == 0 && aligned16(rows) && aligned16(dense))
    hipLaunchKernelGGL((dense_move_h<8, kGather>), FV2P_GRID1D(n * (c / 8)), 0, s, ind, (int)n, c, ndim, d1, d2, vol, 0, static_cast<u16*>(rows), static_cast<u16*>(dense));
  else
    hipLaunchKernelGGL((dense_move_h<1, kGather>), FV2P_GRID1D(n * c), 0, s, ind, (int)n, c, ndim, d1, d2, vol, channels_first ? 1 : 0, static_cast<u16*>(rows),
                       static_cast<u16*>(dense));
}
extern "C" int fv2p_sparse_to_dense_h(const void* features, const int* indices, int64_t n, int c, int ndim, int batch, const int spatial[3],
                                      int channels_first, void* dense, int dtype, fv2p_stream_t s_) {
  hipStream_t s = static_cast<hipStream_t>(s_);
  FV2P_DT16_OK("sparse_to_dense_h", dtype);
  FV2P_REQUIRE(c >= 1 && n >= 0 && n < (1ll << 31) && batch >= 1 && (ndim == 2 || ndim == 3), FV2P_EINVAL, "sparse_to_dense_h: bad sizes");
  FV2P_REQUIRE(dense && spatial, FV2P_EINVAL, "sparse_to_dense_h: null pointer");
  FV2P_REQUIRE(n == 0 || (features && indices), FV2P_EINVAL, "sparse_to_dense_h: null pointer");
  const int64_t vol = ndim == 3 ? static_cast<int64_t>(spatial[0]) * spatial[1] * spatial[2] : static_cast<int64_t>(spatial[0]) * spatial[1];
  FV2P_REQUIRE(vol >= 0, FV2P_EINVAL, "sparse_to_dense_h: bad sizes");
  if (vol > 0) FV2P_HIP(hipMemsetAsync(dense, 0, sizeof(u16) * static_cast<size_t>(batch) * c * vol, s));   // (an odd element count is no multiple of multi_fill's 4 bytes)
  if (n == 0) return 0;
  launch_dense_move_h<false>(indices, n, c, ndim, spatial, vol, channels_first, const_cast<void*>(features), dense, s);
  FV2P_LAUNCH_CHECK();
  return 0;
}
extern "C" int fv2p_dense_to_sparse_h(const void* dense, const int* indices, int64_t n, int c, int ndim, int batch, const int spatial[3],
                                      int channels_first, void* rows, int dtype, fv2p_stream_t s_) {
  hipStream_t s = static_cast<hipStream_t>(s_);
  FV2P_DT16_OK("dense_to_sparse_h", dtype);
  FV2P_REQUIRE(c >= 1 && n >= 0 && n < (1ll << 31) && batch >= 1 && (ndim == 2 || ndim == 3), FV2P_EINVAL, "dense_to_sparse_h: bad sizes");
  FV2P_REQUIRE(n == 0 || (dense && indices && rows && spatial), FV2P_EINVAL, "dense_to_sparse_h: null pointer");
  if (n == 0) return 0;
  const int64_t vol = ndim == 3 ? static_cast<int64_t>(spatial[0]) * spatial[1] * spatial[2] : static_cast<int64_t>(spatial[0]) * spatial[1];
  launch_dense_move_h<true>(indices, n, c, ndim, spatial, vol, channels_first, rows, const_cast<void*>(dense), s);
  FV2P_LAUNCH_CHECK();
  return 0;
}
extern "C" int fv2p_voxel_mean_collate(const float* voxels, const int* coors, const int* num_points, const int* num_voxels,
                                       int max_voxels, int max_points, int ndim, int batch_idx, float* feats, int* coords,
                                       fv2p_stream_t s_) {
  hipStream_t s = static_cast<hipStream_t>(s_);
  FV2P_REQUIRE(max_voxels >= 0 && max_points >= 1 && ndim >= 3, FV2P_EINVAL, "voxel_mean_collate: bad sizes");
  if (max_voxels == 0) return 0;
  FV2P_REQUIRE(voxels && coors && num_points && num_voxels && feats && coords, FV2P_EINVAL, "voxel_mean_collate: null pointer");
  hipLaunchKernelGGL(voxel_mean_collate, FV2P_GRID1D(static_cast<int64_t>(max_voxels) * ndim), 0, s, voxels, coors, num_points, num_voxels,
                     max_voxels, max_points, ndim, batch_idx, feats, coords);
  FV2P_LAUNCH_CHECK();
  return 0;
}
