// BatchNorm2d (+ ReLU) on contiguous float16 / bfloat16 NCHW maps [n, c, hw]: the layer of batchnorm2d.hip on the 16-bit volume that
// SparseConvTensor.dense() writes and the BEV backbones' convolutions keep, with no fp32 image of any map.
//
// The structure is that of batchnorm2d.hip (bn2d_common.hpp): two launches per direction on one grid of (sample, channel, chunk of
// kBn2dChunk16 plane elements) workgroups, one fp64 pair per workgroup from the reduce launch, folded in bn2d_fold's fixed order by
// every workgroup of the apply launch while its own chunk's loads are in flight.  The kernel boundary is the only synchronisation: no
// float atomics, no grid barrier, no last-workgroup protocol; two runs give the same bits.
// The conventions are those of the 16-bit row op (batchnorm_h.hip, dt16.hpp): elements are widened on load, the arithmetic is fp32 (the
// sums fp64), and ONE rounding to nearest even happens at the store.  A thread moves 8 elements per 16-byte access when hw % 8 == 0
// and the maps are 16-byte aligned, one element otherwise.  Parameters (gamma, beta, running statistics, dgamma, dbeta) are fp32 or the
// map's format (`pd`): widened on read, written from the fp64 value with a single rounding.  mean / invstd are always fp32.
// The backward's ReLU mask is the mask of the STORED output, widen(round(t)) > 0, recomputed from x: a float16 pre-activation below
// 2^-25 was stored as 0 and gets no gradient, as threshold_backward on the stored tensor gives none.
#include "bn2d_common.hpp"
#include "dt16.hpp"

namespace fv2p {
namespace {

constexpr int kBn2dChunk16 = 4096;   // plane elements per workgroup: 256 threads x 2 units of 8; norm.py BN2D_CHUNK16 mirrors it
static_assert(kBn2dChunk16 == kBn2dChunk, "bn2d_where / bn2d_geom cut the plane into kBn2dChunk elements");

template <class T, int V>
struct Chunk16 {   // a workgroup's chunk, widened, in registers: thread t holds the V-element units t, t + 256, ...
  static constexpr int U = kBn2dChunk16 / (256 * V);
  float v[U][V];
  __device__ __forceinline__ void load(const u16* __restrict__ p, int len) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int o = (u * 256 + static_cast<int>(threadIdx.x)) * V;
      Row16<T, V> r;
#pragma unroll
      for (int i = 0; i < V; ++i) r.v[i] = 0.f;
      if (o < len) r.load(p + o);   // len % 8 == 0 on the vector path
#pragma unroll
      for (int i = 0; i < V; ++i) v[u][i] = r.v[i];
    }
  }
  __device__ __forceinline__ void store(u16* __restrict__ p, int len) const {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int o = (u * 256 + static_cast<int>(threadIdx.x)) * V;
      if (o < len) {
        Row16<T, V> r;
#pragma unroll
        for (int i = 0; i < V; ++i) r.v[i] = v[u][i];
        r.store(p + o);
      }
    }
  }
};

// dz where the STORED output is positive (y: the fp32 value the forward rounded), dz everywhere without a ReLU
template <class T>
__device__ __forceinline__ float bn2d_masked(float y, float dz, int relu) {
  return (relu && !(T::widen(T::round(y)) > 0.f)) ? 0.f : dz;
}

// partial: [c][parts][2] doubles.  BWD: mean / invstd / gamma / beta of the forward pass, dz the gradient of the layer's output.
template <class T, int V, bool BWD>
__global__ __launch_bounds__(256) void bn2d_reduce_h_k(const u16* __restrict__ x, const u16* __restrict__ dz, Bn2dGeom g,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd,
                                                       const void* __restrict__ gamma, const void* __restrict__ beta, int pd, int relu,
                                                       double* __restrict__ partial, const long long* __restrict__ nbt,
                                                       long long* __restrict__ nbt_copy) {
  __shared__ double red[2][4];
  const Bn2dWhere w = bn2d_where(g);
  if (!BWD && nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt_copy = *nbt;
  Chunk16<T, V> xv;
  xv.load(x + w.off, w.len);
  double a = 0.0, b = 0.0;
  if constexpr (!BWD) {
    // (elements past the chunk's end were loaded as zeros: they add nothing)
#pragma unroll
    for (int u = 0; u < Chunk16<T, V>::U; ++u)
#pragma unroll
      for (int i = 0; i < V; ++i) { const double d = xv.v[u][i]; a += d; b += d * d; }
  } else {
    Chunk16<T, V> gv;
    gv.load(dz + w.off, w.len);   // zeros past the end: dy = 0 there
    const float mu = mean[w.ch], is = invstd[w.ch], ga = par_load<T>(gamma, w.ch, pd, 1.f), be = par_load<T>(beta, w.ch, pd, 0.f);
#pragma unroll
    for (int u = 0; u < Chunk16<T, V>::U; ++u)
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float xhat;
        const float y = bn2d_act(xv.v[u][i], mu, is, ga, be, relu, &xhat);
        const float dy = bn2d_masked<T>(y, gv.v[u][i], relu);
        a += dy; b += static_cast<double>(dy) * xhat;
      }
  }
  bn2d_block_sum(a, b, red);
  if (threadIdx.x == 0) {
    double* p = partial + (static_cast<long long>(w.ch) * g.parts + w.part) * 2;
    p[0] = a; p[1] = b;
  }
}

struct Bn2dRun {   // running statistics in the parameters' format (fp32 or T)
  void* running_mean; void* running_var; long long* num_batches_tracked;
};

// FOLD: batch statistics from the partials (training); otherwise mean / invstd are read from memory (eval mode).
template <class T, int V, bool FOLD>
__global__ __launch_bounds__(256) void bn2d_apply_fwd_h_k(const u16* __restrict__ x, Bn2dGeom g, const double* __restrict__ partial,
                                                          const long long* __restrict__ nbt_copy, float* __restrict__ mean,
                                                          float* __restrict__ invstd, Bn2dRun run, float eps, float momentum,
                                                          const void* __restrict__ gamma, const void* __restrict__ beta, int pd, int relu,
                                                          u16* __restrict__ y) {
  __shared__ double red[2][4];
  __shared__ float sh_stat[2];
  const Bn2dWhere w = bn2d_where(g);
  Chunk16<T, V> xv;
  xv.load(x + w.off, w.len);   // in flight while the partials are folded
  float mu, is;
  if constexpr (FOLD) {
    double a, b;
    bn2d_fold(partial, g, w.ch, red, &a, &b);
    if (threadIdx.x == 0) {
      const double m = a / g.count;
      double var = b / g.count - m * m;
      if (var < 0.0) var = 0.0;
      const float mu_f = static_cast<float>(m), is_f = static_cast<float>(1.0 / sqrt(var + static_cast<double>(eps)));
      sh_stat[0] = mu_f; sh_stat[1] = is_f;
      if (w.first) {
        mean[w.ch] = mu_f;
        invstd[w.ch] = is_f;
        if (run.running_mean) {
          const long long seen = run.num_batches_tracked ? *nbt_copy : 0;   // the value before this call's bump
          const double f = momentum < 0.f ? 1.0 / static_cast<double>(seen + 1) : static_cast<double>(momentum);
          const double unbiased = g.count > 1.0 ? var * g.count / (g.count - 1.0) : var;
          // the update on the (widened) old values in fp64, rounded once to the parameters' format
          const double rm = par_load<T>(run.running_mean, w.ch, pd, 0.f), rv = par_load<T>(run.running_var, w.ch, pd, 0.f);
          par_store<T>(run.running_mean, w.ch, pd, (1.0 - f) * rm + f * m);
          par_store<T>(run.running_var, w.ch, pd, (1.0 - f) * rv + f * unbiased);
          if (w.ch == 0 && run.num_batches_tracked) *run.num_batches_tracked = seen + 1;
        }
      }
    }
    __syncthreads();
    mu = sh_stat[0]; is = sh_stat[1];
  } else {
    mu = mean[w.ch]; is = invstd[w.ch];
  }
  const float ga = par_load<T>(gamma, w.ch, pd, 1.f), be = par_load<T>(beta, w.ch, pd, 0.f);
#pragma unroll
  for (int u = 0; u < Chunk16<T, V>::U; ++u)
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float xhat;
      xv.v[u][i] = bn2d_act(xv.v[u][i], mu, is, ga, be, relu, &xhat);
    }
  xv.store(y + w.off, w.len);   // the ONE rounding
}

template <class T, int V>
__global__ __launch_bounds__(256) void bn2d_apply_bwd_h_k(const u16* __restrict__ x, const u16* __restrict__ dz, Bn2dGeom g,
                                                          const double* __restrict__ partial, const float* __restrict__ mean,
                                                          const float* __restrict__ invstd, const void* __restrict__ gamma,
                                                          const void* __restrict__ beta, int pd, int relu, int batch_stats,
                                                          void* __restrict__ dgamma, void* __restrict__ dbeta, u16* __restrict__ dx) {
  __shared__ double red[2][4];
  __shared__ float sh_coef[2];
  const Bn2dWhere w = bn2d_where(g);
  Chunk16<T, V> xv, gv;
  xv.load(x + w.off, w.len);
  gv.load(dz + w.off, w.len);
  double a, b;
  bn2d_fold(partial, g, w.ch, red, &a, &b);
  if (threadIdx.x == 0) {
    if (w.first) { par_store<T>(dbeta, w.ch, pd, a); par_store<T>(dgamma, w.ch, pd, b); }
    sh_coef[0] = batch_stats ? static_cast<float>(a / g.count) : 0.f;
    sh_coef[1] = batch_stats ? static_cast<float>(b / g.count) : 0.f;
  }
  __syncthreads();
  const float c1 = sh_coef[0], c2 = sh_coef[1];
  const float mu = mean[w.ch], is = invstd[w.ch], ga = par_load<T>(gamma, w.ch, pd, 1.f), be = par_load<T>(beta, w.ch, pd, 0.f);
#pragma unroll
  for (int u = 0; u < Chunk16<T, V>::U; ++u)
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float xhat;
      const float y = bn2d_act(xv.v[u][i], mu, is, ga, be, relu, &xhat);
      const float dy = bn2d_masked<T>(y, gv.v[u][i], relu);
      xv.v[u][i] = ga * is * (dy - c1 - xhat * c2);
    }
  xv.store(dx + w.off, w.len);
}

struct FwdArgs2d {
  const u16* x; Bn2dGeom g; const double* partial; const long long* nbt; long long* nbt_copy; float* mean; float* invstd; Bn2dRun run;
  float eps, momentum; const void* gamma; const void* beta; int pd, relu; u16* y;
};
template <class T, int V>
void launch_fwd2d(const FwdArgs2d& a, bool fold, hipStream_t stream) {
  const unsigned grid = bn2d_grid(a.g);
  if (fold) {
    hipLaunchKernelGGL((bn2d_reduce_h_k<T, V, false>), dim3(grid), dim3(256), 0, stream, a.x, nullptr, a.g, nullptr, nullptr, nullptr, nullptr, 0, 0,
                       const_cast<double*>(a.partial), a.nbt, a.nbt_copy);
    hipLaunchKernelGGL((bn2d_apply_fwd_h_k<T, V, true>), dim3(grid), dim3(256), 0, stream, a.x, a.g, a.partial, a.nbt_copy, a.mean, a.invstd, a.run,
                       a.eps, a.momentum, a.gamma, a.beta, a.pd, a.relu, a.y);
  } else {
    hipLaunchKernelGGL((bn2d_apply_fwd_h_k<T, V, false>), dim3(grid), dim3(256), 0, stream, a.x, a.g, nullptr, nullptr, a.mean, a.invstd, a.run,
                       a.eps, a.momentum, a.gamma, a.beta, a.pd, a.relu, a.y);
  }
}

struct BwdArgs2d {
  const u16* x; const u16* dz; Bn2dGeom g; double* partial; const float* mean; const float* invstd; const void* gamma; const void* beta;
  int pd, relu, batch_stats; void* dgamma; void* dbeta; u16* dx;
};
template <class T, int V>
void launch_bwd2d(const BwdArgs2d& a, hipStream_t stream) {
  const unsigned grid = bn2d_grid(a.g);
  hipLaunchKernelGGL((bn2d_reduce_h_k<T, V, true>), dim3(grid), dim3(256), 0, stream, a.x, a.dz, a.g, a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu,
                     a.partial, nullptr, nullptr);
  hipLaunchKernelGGL((bn2d_apply_bwd_h_k<T, V>), dim3(grid), dim3(256), 0, stream, a.x, a.dz, a.g, a.partial, a.mean, a.invstd, a.gamma, a.beta, a.pd,
                     a.relu, a.batch_stats, a.dgamma, a.dbeta, a.dx);
}

// the four (format, width) instances of a launcher
#define FV2P_BN2D_H_DISPATCH(fn, ...)                                       \
  do {                                                                      \
    if (dtype == FV2P_DT_F16) { if (vec) fn<H16, 8>(__VA_ARGS__); else fn<H16, 1>(__VA_ARGS__); } \
    else { if (vec) fn<B16, 8>(__VA_ARGS__); else fn<B16, 1>(__VA_ARGS__); }                      \
  } while (0)

}  // namespace
}  // namespace fv2p

using namespace fv2p;

#define FV2P_BN2D_H_DTYPES(name)                                                                                                                \
  FV2P_DT16_OK(name, dtype);                                                                                                                    \
  FV2P_REQUIRE(param_dtype == 0 || param_dtype == dtype, FV2P_EINVAL, name ": param_dtype %d is neither 0 (fp32) nor the call's dtype %d",     \
               param_dtype, dtype)

extern "C" size_t fv2p_batchnorm2d_h_ws_bytes(int64_t n, int c, int64_t hw) {
  Bn2dGeom g;
  if (n < 1 || c < 1 || hw < 1 || bn2d_geom(n, c, hw, &g)) return 0;
  Sizer s;
  bn2d_ws(s, g);   // the fp64 partials and the counter copy: nothing of the map's size
  return s.bytes();
}

extern "C" int fv2p_batchnorm2d_forward_h(const void* x, int64_t n, int c, int64_t hw, float eps, float momentum, const void* gamma,
                                          const void* beta, int relu, void* running_mean, void* running_var, int64_t* num_batches_tracked,
                                          float* mean, float* invstd, void* y, int dtype, int param_dtype, void* ws, size_t ws_bytes,
                                          fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FV2P_BN2D_H_DTYPES("batchnorm2d_forward_h");
  FV2P_REQUIRE(n >= 1 && c >= 1 && hw >= 1, FV2P_EINVAL, "batchnorm2d_forward_h: n=%lld c=%d hw=%lld", static_cast<long long>(n), c, static_cast<long long>(hw));
  FV2P_REQUIRE(x && y && mean && invstd && ws, FV2P_EINVAL, "batchnorm2d_forward_h: null pointer");
  FV2P_REQUIRE((running_mean == nullptr) == (running_var == nullptr), FV2P_EINVAL, "batchnorm2d_forward_h: running_mean and running_var come together");
  Bn2dGeom g;
  const char* why = bn2d_geom(n, c, hw, &g);
  FV2P_REQUIRE(!why, FV2P_ELIMIT, "batchnorm2d_forward_h: too many %s (n=%lld c=%d hw=%lld)", why, static_cast<long long>(n), c, static_cast<long long>(hw));
  FV2P_REQUIRE(ws_bytes >= fv2p_batchnorm2d_h_ws_bytes(n, c, hw), FV2P_EWORKSPACE, "batchnorm2d_forward_h: workspace %lld < %lld",
               static_cast<long long>(ws_bytes), static_cast<long long>(fv2p_batchnorm2d_h_ws_bytes(n, c, hw)));
  Carver cv(ws, ws_bytes);
  const Bn2dWs w = bn2d_ws(cv, g);
  FwdArgs2d a;
  a.x = static_cast<const u16*>(x); a.g = g; a.partial = w.partial; a.nbt_copy = w.nbt_copy;
  a.nbt = reinterpret_cast<const long long*>(running_mean ? num_batches_tracked : nullptr);
  a.mean = mean; a.invstd = invstd;
  a.run = Bn2dRun{running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked)};
  a.eps = eps; a.momentum = momentum; a.gamma = gamma; a.beta = beta; a.pd = param_dtype != 0; a.relu = relu; a.y = static_cast<u16*>(y);
  const bool vec = hw % 8 == 0 && aligned16(x) && aligned16(y);
  FV2P_BN2D_H_DISPATCH(launch_fwd2d, a, true, stream);
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" int fv2p_batchnorm2d_apply_h(const void* x, int64_t n, int c, int64_t hw, const float* mean, const float* invstd, const void* gamma,
                                        const void* beta, int relu, void* y, int dtype, int param_dtype, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FV2P_BN2D_H_DTYPES("batchnorm2d_apply_h");
  FV2P_REQUIRE(n >= 0 && c >= 1 && hw >= 0, FV2P_EINVAL, "batchnorm2d_apply_h: n=%lld c=%d hw=%lld", static_cast<long long>(n), c, static_cast<long long>(hw));
  if (n == 0 || hw == 0) return 0;
  FV2P_REQUIRE(x && y && mean && invstd, FV2P_EINVAL, "batchnorm2d_apply_h: null pointer");
  Bn2dGeom g;
  const char* why = bn2d_geom(n, c, hw, &g);
  FV2P_REQUIRE(!why, FV2P_ELIMIT, "batchnorm2d_apply_h: too many %s (n=%lld c=%d hw=%lld)", why, static_cast<long long>(n), c, static_cast<long long>(hw));
  FwdArgs2d a;
  a.x = static_cast<const u16*>(x); a.g = g; a.partial = nullptr; a.nbt = nullptr; a.nbt_copy = nullptr;
  a.mean = const_cast<float*>(mean); a.invstd = const_cast<float*>(invstd);
  a.run = Bn2dRun{nullptr, nullptr, nullptr};
  a.eps = 0.f; a.momentum = 0.f; a.gamma = gamma; a.beta = beta; a.pd = param_dtype != 0; a.relu = relu; a.y = static_cast<u16*>(y);
  const bool vec = hw % 8 == 0 && aligned16(x) && aligned16(y);
  FV2P_BN2D_H_DISPATCH(launch_fwd2d, a, false, stream);
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" int fv2p_batchnorm2d_backward_h(const void* x, const void* dz, int64_t n, int c, int64_t hw, const float* mean, const float* invstd,
                                           const void* gamma, const void* beta, int relu, int batch_stats, void* dx, void* dgamma, void* dbeta,
                                           int dtype, int param_dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FV2P_BN2D_H_DTYPES("batchnorm2d_backward_h");
  FV2P_REQUIRE(n >= 1 && c >= 1 && hw >= 1, FV2P_EINVAL, "batchnorm2d_backward_h: n=%lld c=%d hw=%lld", static_cast<long long>(n), c, static_cast<long long>(hw));
  FV2P_REQUIRE(x && dz && mean && invstd && dx && dgamma && dbeta && ws, FV2P_EINVAL, "batchnorm2d_backward_h: null pointer");
  Bn2dGeom g;
  const char* why = bn2d_geom(n, c, hw, &g);
  FV2P_REQUIRE(!why, FV2P_ELIMIT, "batchnorm2d_backward_h: too many %s (n=%lld c=%d hw=%lld)", why, static_cast<long long>(n), c, static_cast<long long>(hw));
  FV2P_REQUIRE(ws_bytes >= fv2p_batchnorm2d_h_ws_bytes(n, c, hw), FV2P_EWORKSPACE, "batchnorm2d_backward_h: workspace %lld < %lld",
               static_cast<long long>(ws_bytes), static_cast<long long>(fv2p_batchnorm2d_h_ws_bytes(n, c, hw)));
  Carver cv(ws, ws_bytes);
  const Bn2dWs w = bn2d_ws(cv, g);
  BwdArgs2d a;
  a.x = static_cast<const u16*>(x); a.dz = static_cast<const u16*>(dz); a.g = g; a.partial = w.partial; a.mean = mean; a.invstd = invstd;
  a.gamma = gamma; a.beta = beta; a.pd = param_dtype != 0; a.relu = relu; a.batch_stats = batch_stats;
  a.dgamma = dgamma; a.dbeta = dbeta; a.dx = static_cast<u16*>(dx);
  const bool vec = hw % 8 == 0 && aligned16(x) && aligned16(dz) && aligned16(dx);
  FV2P_BN2D_H_DISPATCH(launch_bwd2d, a, stream);
  FV2P_LAUNCH_CHECK();
  return 0;
}
