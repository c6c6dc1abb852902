// BatchNorm2d (+ ReLU) on contiguous fp32 NCHW maps [n, c, hw] - the pair behind every Conv2d / ConvTranspose2d of the reference's BEV
// backbones (pcdet/models/backbones_2d/base_bev_backbone.py:27-60: nn.BatchNorm2d(eps=1e-3, momentum=0.01), nn.ReLU()).
//
// torch runs the pair as MIOpen's spatial BatchNorm (reads x twice, writes) and an elementwise clamp (reads, writes): 5 passes over the
// map forward, 8 backward (threshold_backward 3, BatchNorm backward 5).  Here the layer is two launches per direction, 3 passes forward
// and 5 backward, and the pre-activation tensor does not exist:
//   forward : bn2d_reduce_k<FWD>   one workgroup per (sample, channel, chunk of kBn2dChunk plane elements): sum x, sum x^2 in fp64 ->
//                                  partial[channel][sample * chunks + chunk][2]
//             bn2d_apply_fwd_k     same grid; every workgroup loads its chunk, folds the partials of ITS channel in one fixed order,
//                                  derives mean / invstd and writes y = relu?((x - mean) * invstd * gamma + beta); the workgroup of
//                                  (sample 0, chunk 0) of a channel also stores mean / invstd and moves the running statistics
//   backward: bn2d_reduce_k<BWD>   dy = dz * [y > 0] with y recomputed from x (bn2d_act, the forward's own expression: same bits);
//                                  sum dy, sum dy * xhat
//             bn2d_apply_bwd_k     folds to dbeta, dgamma, c1, c2;  dx = gamma * invstd * (dy - c1 - xhat * c2)
// Nothing crosses workgroups inside a launch: no atomics, no counters, no waiting.  The kernel boundary is the synchronisation, and
// the fold order depends on the shape alone, so two runs give the same bits.
// num_batches_tracked (momentum < 0: cumulative average) is read by every channel's finalising workgroup; the reduce launch copies it
// into the workspace and the apply launch reads that copy, so the bump (by channel 0's finalising workgroup) cannot overtake a reader.
#include "bn2d_common.hpp"   // the grid, the fold, bn2d_act and the workspace layout, shared with batchnorm2d_h.hip

namespace fv2p {

template <int V>
struct Chunk {   // a workgroup's chunk in registers: thread t holds the V-element units t, t + 256, ...
  static constexpr int U = kBn2dChunk / (256 * V);
  float v[U][V];
  __device__ __forceinline__ void load(const float* __restrict__ p, int len) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int o = (u * 256 + static_cast<int>(threadIdx.x)) * V;
      if constexpr (V == 4) {
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (o < len) q = *reinterpret_cast<const float4*>(p + o);   // len % 4 == 0 on this path
        v[u][0] = q.x; v[u][1] = q.y; v[u][2] = q.z; v[u][3] = q.w;
      } else {
        v[u][0] = o < len ? p[o] : 0.f;
      }
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ p, int len) const {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int o = (u * 256 + static_cast<int>(threadIdx.x)) * V;
      if (o < len) {
        if constexpr (V == 4) *reinterpret_cast<float4*>(p + o) = make_float4(v[u][0], v[u][1], v[u][2], v[u][3]);
        else p[o] = v[u][0];
      }
    }
  }
};

// partial: [c][parts][2] doubles.  BWD: mean / invstd / gamma / beta of the forward pass, dz the gradient of the layer's output.
template <int V, bool BWD>
__global__ __launch_bounds__(256) void bn2d_reduce_k(const float* __restrict__ x, const float* __restrict__ dz, Bn2dGeom g,
                                                     const float* __restrict__ mean, const float* __restrict__ invstd,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, int relu,
                                                     double* __restrict__ partial, const long long* __restrict__ nbt, long long* __restrict__ nbt_copy) {
  __shared__ double red[2][4];
  const Bn2dWhere w = bn2d_where(g);
  if (!BWD && nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt_copy = *nbt;
  Chunk<V> xv, gv;
  xv.load(x + w.off, w.len);
  double a = 0.0, b = 0.0;
  if constexpr (!BWD) {
    // (elements past the chunk's end were loaded as zeros: they add nothing)
#pragma unroll
    for (int u = 0; u < Chunk<V>::U; ++u)
#pragma unroll
      for (int i = 0; i < V; ++i) { const double d = xv.v[u][i]; a += d; b += d * d; }
  } else {
    gv.load(dz + w.off, w.len);   // zeros past the end: dy = 0 there
    const float mu = mean[w.ch], is = invstd[w.ch], ga = gamma ? gamma[w.ch] : 1.f, be = beta ? beta[w.ch] : 0.f;
#pragma unroll
    for (int u = 0; u < Chunk<V>::U; ++u)
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float xhat;
        const float y = bn2d_act(xv.v[u][i], mu, is, ga, be, relu, &xhat);
        const float dy = (relu && !(y > 0.f)) ? 0.f : gv.v[u][i];
        a += dy; b += static_cast<double>(dy) * xhat;
      }
  }
  bn2d_block_sum(a, b, red);
  if (threadIdx.x == 0) {
    double* p = partial + (static_cast<long long>(w.ch) * g.parts + w.part) * 2;
    p[0] = a; p[1] = b;
  }
}

// FOLD: batch statistics from the partials (training); otherwise mean / invstd are read from ff (eval mode).
template <int V, bool FOLD>
__global__ __launch_bounds__(256) void bn2d_apply_fwd_k(const float* __restrict__ x, Bn2dGeom g, const double* __restrict__ partial,
                                                        const long long* __restrict__ nbt_copy, BnFwdFin ff, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int relu, float* __restrict__ y) {
  __shared__ double red[2][4];
  __shared__ float sh_stat[2];
  const Bn2dWhere w = bn2d_where(g);
  Chunk<V> xv;
  xv.load(x + w.off, w.len);   // in flight while the partials are folded
  float mu, is;
  if constexpr (FOLD) {
    double a, b;
    bn2d_fold(partial, g, w.ch, red, &a, &b);
    if (threadIdx.x == 0) {
      const double m = a / g.count;
      double var = b / g.count - m * m;
      if (var < 0.0) var = 0.0;
      const float mu_f = static_cast<float>(m), is_f = static_cast<float>(1.0 / sqrt(var + static_cast<double>(ff.eps)));
      sh_stat[0] = mu_f; sh_stat[1] = is_f;
      if (w.first) {
        ff.mean[w.ch] = mu_f;
        ff.invstd[w.ch] = is_f;
        if (ff.running_mean) {
          const long long seen = ff.num_batches_tracked ? *nbt_copy : 0;   // the value before this call's bump
          const double f = ff.momentum < 0.f ? 1.0 / static_cast<double>(seen + 1) : static_cast<double>(ff.momentum);
          const double unbiased = g.count > 1.0 ? var * g.count / (g.count - 1.0) : var;
          ff.running_mean[w.ch] = static_cast<float>((1.0 - f) * ff.running_mean[w.ch] + f * m);
          ff.running_var[w.ch] = static_cast<float>((1.0 - f) * ff.running_var[w.ch] + f * unbiased);
          if (w.ch == 0 && ff.num_batches_tracked) *ff.num_batches_tracked = seen + 1;
        }
      }
    }
    __syncthreads();
    mu = sh_stat[0]; is = sh_stat[1];
  } else {
    mu = ff.mean[w.ch]; is = ff.invstd[w.ch];
  }
  const float ga = gamma ? gamma[w.ch] : 1.f, be = beta ? beta[w.ch] : 0.f;
#pragma unroll
  for (int u = 0; u < Chunk<V>::U; ++u)
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float xhat;
      xv.v[u][i] = bn2d_act(xv.v[u][i], mu, is, ga, be, relu, &xhat);
    }
  xv.store(y + w.off, w.len);
}

template <int V>
__global__ __launch_bounds__(256) void bn2d_apply_bwd_k(const float* __restrict__ x, const float* __restrict__ dz, Bn2dGeom g,
                                                        const double* __restrict__ partial, const float* __restrict__ mean,
                                                        const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int relu, int batch_stats, float* __restrict__ dgamma,
                                                        float* __restrict__ dbeta, float* __restrict__ dx) {
  __shared__ double red[2][4];
  __shared__ float sh_coef[2];
  const Bn2dWhere w = bn2d_where(g);
  Chunk<V> xv, gv;
  xv.load(x + w.off, w.len);
  gv.load(dz + w.off, w.len);
  double a, b;
  bn2d_fold(partial, g, w.ch, red, &a, &b);
  if (threadIdx.x == 0) {
    if (w.first) { dbeta[w.ch] = static_cast<float>(a); dgamma[w.ch] = static_cast<float>(b); }
    sh_coef[0] = batch_stats ? static_cast<float>(a / g.count) : 0.f;
    sh_coef[1] = batch_stats ? static_cast<float>(b / g.count) : 0.f;
  }
  __syncthreads();
  const float c1 = sh_coef[0], c2 = sh_coef[1];
  const float mu = mean[w.ch], is = invstd[w.ch], ga = gamma ? gamma[w.ch] : 1.f, be = beta ? beta[w.ch] : 0.f;
#pragma unroll
  for (int u = 0; u < Chunk<V>::U; ++u)
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float xhat;
      const float y = bn2d_act(xv.v[u][i], mu, is, ga, be, relu, &xhat);
      const float dy = (relu && !(y > 0.f)) ? 0.f : gv.v[u][i];
      xv.v[u][i] = ga * is * (dy - c1 - xhat * c2);
    }
  xv.store(dx + w.off, w.len);
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace fv2p

using namespace fv2p;

extern "C" size_t fv2p_batchnorm2d_ws_bytes(int64_t n, int c, int64_t hw) {
  Bn2dGeom g;
  if (n < 1 || c < 1 || hw < 1 || bn2d_geom(n, c, hw, &g)) return 0;
  Sizer s;
  bn2d_ws(s, g);
  return s.bytes();
}

extern "C" int fv2p_batchnorm2d_forward(const float* x, int64_t n, int c, int64_t hw, float eps, float momentum, const float* gamma,
                                        const float* beta, int relu, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                        float* mean, float* invstd, float* y, void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FV2P_REQUIRE(n >= 1 && c >= 1 && hw >= 1, FV2P_EINVAL, "batchnorm2d_forward: n=%lld c=%d hw=%lld", static_cast<long long>(n), c, static_cast<long long>(hw));
  FV2P_REQUIRE(x && y && mean && invstd && ws, FV2P_EINVAL, "batchnorm2d_forward: null pointer");
  FV2P_REQUIRE((running_mean == nullptr) == (running_var == nullptr), FV2P_EINVAL, "batchnorm2d_forward: running_mean and running_var come together");
  Bn2dGeom g;
  const char* why = bn2d_geom(n, c, hw, &g);
  FV2P_REQUIRE(!why, FV2P_ELIMIT, "batchnorm2d_forward: too many %s (n=%lld c=%d hw=%lld)", why, static_cast<long long>(n), c, static_cast<long long>(hw));
  FV2P_REQUIRE(ws_bytes >= fv2p_batchnorm2d_ws_bytes(n, c, hw), FV2P_EWORKSPACE, "batchnorm2d_forward: workspace %lld < %lld",
               static_cast<long long>(ws_bytes), static_cast<long long>(fv2p_batchnorm2d_ws_bytes(n, c, hw)));
  Carver cv(ws, ws_bytes);
  const Bn2dWs w = bn2d_ws(cv, g);
  const long long* nbt = reinterpret_cast<const long long*>(running_mean ? num_batches_tracked : nullptr);
  BnFwdFin ff{mean, invstd, running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked), momentum, eps};
  const unsigned grid = bn2d_grid(g);
  if (hw % 4 == 0 && aligned16(x) && aligned16(y)) {
    hipLaunchKernelGGL((bn2d_reduce_k<4, false>), dim3(grid), dim3(256), 0, stream, x, nullptr, g, nullptr, nullptr, nullptr, nullptr, 0, w.partial, nbt, w.nbt_copy);
    hipLaunchKernelGGL((bn2d_apply_fwd_k<4, true>), dim3(grid), dim3(256), 0, stream, x, g, w.partial, w.nbt_copy, ff, gamma, beta, relu, y);
  } else {
    hipLaunchKernelGGL((bn2d_reduce_k<1, false>), dim3(grid), dim3(256), 0, stream, x, nullptr, g, nullptr, nullptr, nullptr, nullptr, 0, w.partial, nbt, w.nbt_copy);
    hipLaunchKernelGGL((bn2d_apply_fwd_k<1, true>), dim3(grid), dim3(256), 0, stream, x, g, w.partial, w.nbt_copy, ff, gamma, beta, relu, y);
  }
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" int fv2p_batchnorm2d_apply(const float* x, int64_t n, int c, int64_t hw, const float* mean, const float* invstd, const float* gamma,
                                      const float* beta, int relu, float* y, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FV2P_REQUIRE(n >= 0 && c >= 1 && hw >= 0, FV2P_EINVAL, "batchnorm2d_apply: n=%lld c=%d hw=%lld", static_cast<long long>(n), c, static_cast<long long>(hw));
  if (n == 0 || hw == 0) return 0;
  FV2P_REQUIRE(x && y && mean && invstd, FV2P_EINVAL, "batchnorm2d_apply: null pointer");
  Bn2dGeom g;
  const char* why = bn2d_geom(n, c, hw, &g);
  FV2P_REQUIRE(!why, FV2P_ELIMIT, "batchnorm2d_apply: too many %s (n=%lld c=%d hw=%lld)", why, static_cast<long long>(n), c, static_cast<long long>(hw));
  BnFwdFin ff{const_cast<float*>(mean), const_cast<float*>(invstd), nullptr, nullptr, nullptr, 0.f, 0.f};
  const unsigned grid = bn2d_grid(g);
  if (hw % 4 == 0 && aligned16(x) && aligned16(y))
    hipLaunchKernelGGL((bn2d_apply_fwd_k<4, false>), dim3(grid), dim3(256), 0, stream, x, g, nullptr, nullptr, ff, gamma, beta, relu, y);
  else
    hipLaunchKernelGGL((bn2d_apply_fwd_k<1, false>), dim3(grid), dim3(256), 0, stream, x, g, nullptr, nullptr, ff, gamma, beta, relu, y);
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" int fv2p_batchnorm2d_backward(const float* x, const float* dz, int64_t n, int c, int64_t hw, const float* mean, const float* invstd,
                                         const float* gamma, const float* beta, int relu, int batch_stats, float* dx, float* dgamma,
                                         float* dbeta, void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FV2P_REQUIRE(n >= 1 && c >= 1 && hw >= 1, FV2P_EINVAL, "batchnorm2d_backward: n=%lld c=%d hw=%lld", static_cast<long long>(n), c, static_cast<long long>(hw));
  FV2P_REQUIRE(x && dz && mean && invstd && dx && dgamma && dbeta && ws, FV2P_EINVAL, "batchnorm2d_backward: null pointer");
  Bn2dGeom g;
  const char* why = bn2d_geom(n, c, hw, &g);
  FV2P_REQUIRE(!why, FV2P_ELIMIT, "batchnorm2d_backward: too many %s (n=%lld c=%d hw=%lld)", why, static_cast<long long>(n), c, static_cast<long long>(hw));
  FV2P_REQUIRE(ws_bytes >= fv2p_batchnorm2d_ws_bytes(n, c, hw), FV2P_EWORKSPACE, "batchnorm2d_backward: workspace %lld < %lld",
               static_cast<long long>(ws_bytes), static_cast<long long>(fv2p_batchnorm2d_ws_bytes(n, c, hw)));
  Carver cv(ws, ws_bytes);
  const Bn2dWs w = bn2d_ws(cv, g);
  const unsigned grid = bn2d_grid(g);
  if (hw % 4 == 0 && aligned16(x) && aligned16(dz) && aligned16(dx)) {
    hipLaunchKernelGGL((bn2d_reduce_k<4, true>), dim3(grid), dim3(256), 0, stream, x, dz, g, mean, invstd, gamma, beta, relu, w.partial, nullptr, nullptr);
    hipLaunchKernelGGL((bn2d_apply_bwd_k<4>), dim3(grid), dim3(256), 0, stream, x, dz, g, w.partial, mean, invstd, gamma, beta, relu, batch_stats, dgamma, dbeta, dx);
  } else {
    hipLaunchKernelGGL((bn2d_reduce_k<1, true>), dim3(grid), dim3(256), 0, stream, x, dz, g, mean, invstd, gamma, beta, relu, w.partial, nullptr, nullptr);
    hipLaunchKernelGGL((bn2d_apply_bwd_k<1>), dim3(grid), dim3(256), 0, stream, x, dz, g, w.partial, mean, invstd, gamma, beta, relu, batch_stats, dgamma, dbeta, dx);
  }
  FV2P_LAUNCH_CHECK();
  return 0;
}
