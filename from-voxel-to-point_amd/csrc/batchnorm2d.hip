// BatchNorm2d (+ ReLU) on contiguous NCHW maps [n, c, hw] in fp32, float16 or bfloat16 - the pair behind every Conv2d / ConvTranspose2d
// of the reference's BEV backbones (pcdet/models/backbones_2d/base_bev_backbone.py:27-60: nn.BatchNorm2d(eps=1e-3, momentum=0.01),
// nn.ReLU()), on fp32 maps or on the 16-bit volume that SparseConvTensor.dense() writes, with no fp32 image of any map.
//
// torch runs the pair as MIOpen's spatial BatchNorm (reads x twice, writes) and an elementwise clamp (reads, writes): 5 passes over the
// map forward, 8 backward (threshold_backward 3, BatchNorm backward 5).  Here the layer is two launches per direction, 3 passes forward
// and 5 backward, and the pre-activation tensor does not exist:
//   forward : bn2d_reduce_k<FWD>   one workgroup per (sample, channel, chunk of kBn2dChunk plane elements): sum x, sum x^2 in fp64 ->
//                                  partial[channel][sample * chunks + chunk][2]
//             bn2d_apply_fwd_k     same grid; every workgroup loads its chunk, folds the partials of ITS channel in one fixed order,
//                                  derives mean / invstd and writes y = relu?((x - mean) * invstd * gamma + beta); the workgroup of
//                                  (sample 0, chunk 0) of a channel also stores mean / invstd and moves the running statistics
//   backward: bn2d_reduce_k<BWD>   dy = dz * [stored y > 0] with y recomputed from x (bn2d_act, the forward's own expression: same
//                                  bits); sum dy, sum dy * xhat
//             bn2d_apply_bwd_k     folds to dbeta, dgamma, c1, c2;  dx = gamma * invstd * (dy - c1 - xhat * c2)
// Nothing crosses workgroups inside a launch: no atomics, no counters, no waiting.  The kernel boundary is the synchronisation, and
// the fold order depends on the shape alone, so two runs give the same bits.
// num_batches_tracked (momentum < 0: cumulative average) is read by every channel's finalising workgroup; the reduce launch copies it
// into the workspace and the apply launch reads that copy, so the bump (by channel 0's finalising workgroup) cannot overtake a reader.
//
// The kernels are written once and instantiated per storage format F (bn_fmt.hpp: F32, Fmt16<H16>, Fmt16<B16>).  A format supplies the element
// type, the vector width, the unit of V elements that one access moves (widened to fp32 on load, rounded to nearest even ONCE on
// store), `stored` (the fp32 value of y as memory holds it) and how a parameter is read and written.  Everything else - the arithmetic
// in fp32, the sums in fp64, the grid, the fold, the finalisation - is the same code.  A thread moves one 16-byte unit (4 fp32 or 8
// 16-bit elements) when hw is a multiple of that width and the maps are 16-byte aligned, one element otherwise.
// 16-bit maps take their parameters (gamma, beta, running statistics, dgamma, dbeta) in fp32 or in the map's format (`pd`): widened on
// read, written from the fp64 value with a single rounding.  mean / invstd are always fp32.
// The backward's ReLU mask is the mask of the STORED output, stored(t) > 0, recomputed from x: a float16 pre-activation below 2^-25 was
// stored as 0 and gets no gradient, as threshold_backward on the stored tensor gives none.  (fp32: stored(t) = t.)
#include <type_traits>
#include "common.hpp"
#include "bn_fmt.hpp"

namespace fv2p {
namespace {

constexpr int kBn2dChunk = 4096;   // plane elements per workgroup: 256 threads x 16; pcdet/ops/spconv/norm.py BN2D_CHUNK mirrors it

constexpr int64_t kBn2dMaxGrid = (int64_t(1) << 24) - 1;   // 256-thread workgroups: a launch needs gridDim.x * blockDim.x < 2^32

struct Bn2dGeom {
  long long n, hw, chunks;   // chunks per plane
  int c, parts;              // parts = n * chunks partials per channel
  double count;              // n * hw
};

// The forward's value at one element, and xhat beside it.  Used by the forward apply and by both backward kernels: the mask the
// backward pass recomputes is the forward's, bit for bit (the translation unit is built with -ffp-contract=off).
__device__ __forceinline__ float bn2d_act(float x, float mean, float invstd, float gamma, float beta, int relu, float* xhat) {
  *xhat = (x - mean) * invstd;
  const float t = *xhat * gamma + beta;
  return (relu && t <= 0.f) ? 0.f : t;   // a NaN stays a NaN in y (torch.relu); the backward's !(y > 0) gives it no gradient (threshold_backward)
}

struct Bn2dWhere {
  int ch, first;      // first: the channel's finalising workgroup (sample 0, chunk 0)
  long long off;      // element offset of the chunk
  int len, part;      // elements in the chunk, index of its partial among the channel's
};
__device__ __forceinline__ Bn2dWhere bn2d_where(const Bn2dGeom& g) {
  const long long b = blockIdx.x;                    // ((sample * c + channel) * chunks + chunk): consecutive workgroups stream consecutive memory
  const long long k = b % g.chunks, plane = b / g.chunks;
  const long long s = plane / g.c;
  Bn2dWhere w;
  w.ch = static_cast<int>(plane % g.c);
  w.first = (s == 0 && k == 0);
  w.off = plane * g.hw + k * kBn2dChunk;
  const long long left = g.hw - k * kBn2dChunk;
  w.len = static_cast<int>(left < kBn2dChunk ? left : kBn2dChunk);
  w.part = static_cast<int>(s * g.chunks + k);
  return w;
}

// Sum of (a, b) over the workgroup's 256 threads in a fixed order: xor butterfly inside each wave, then the four waves in order.
// Valid in thread 0.  red: [2][4] doubles.
__device__ __forceinline__ void bn2d_block_sum(double& a, double& b, double (*red)[4]) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) { red[0][tid >> 6] = a; red[1][tid >> 6] = b; }
  __syncthreads();
  if (tid == 0) {
    a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

// The two sums of channel ch over all of its partials, in thread 0: thread t takes partials t, t + 256, ... in order, then bn2d_block_sum.
__device__ __forceinline__ void bn2d_fold(const double* __restrict__ partial, const Bn2dGeom& g, int ch, double (*red)[4], double* a_out, double* b_out) {
  const double* p = partial + static_cast<long long>(ch) * g.parts * 2;
  double a = 0.0, b = 0.0;
  for (int q = threadIdx.x; q < g.parts; q += 256) { a += p[2 * q]; b += p[2 * q + 1]; }
  bn2d_block_sum(a, b, red);
  *a_out = a; *b_out = b;
}

template <class F, int V>
struct Chunk {   // a workgroup's chunk, as fp32, in registers: thread t holds the V-element units t, t + 256, ...
  using elem = typename F::elem;
  static constexpr int U = kBn2dChunk / (256 * V);
  float v[U][V];
  __device__ __forceinline__ void load(const elem* __restrict__ p, int len) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int o = (u * 256 + static_cast<int>(threadIdx.x)) * V;
      typename F::template Unit<V> r;
#pragma unroll
      for (int i = 0; i < V; ++i) r.v[i] = 0.f;
      if (o < len) r.load(p + o);   // len % V == 0 on the vector path
#pragma unroll
      for (int i = 0; i < V; ++i) v[u][i] = r.v[i];
    }
  }
  __device__ __forceinline__ void store(elem* __restrict__ p, int len) const {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int o = (u * 256 + static_cast<int>(threadIdx.x)) * V;
      if (o < len) {
        typename F::template Unit<V> r;
#pragma unroll
        for (int i = 0; i < V; ++i) r.v[i] = v[u][i];
        r.store(p + o);   // the ONE rounding of a 16-bit format
      }
    }
  }
};

// dz where the STORED output is positive (y: the fp32 value the forward stored, rounded or not), dz everywhere without a ReLU
template <class F>
__device__ __forceinline__ float bn2d_masked(float y, float dz, int relu) {
  return (relu && !(F::stored(y) > 0.f)) ? 0.f : dz;
}

// partial: [c][parts][2] doubles.  BWD: mean / invstd / gamma / beta of the forward pass, dz the gradient of the layer's output.
template <class F, int V, bool BWD>
__global__ __launch_bounds__(256) void bn2d_reduce_k(const typename F::elem* __restrict__ x, const typename F::elem* __restrict__ dz, Bn2dGeom g,
                                                     const float* __restrict__ mean, const float* __restrict__ invstd,
                                                     const void* __restrict__ gamma, const void* __restrict__ beta, int pd, int relu,
                                                     double* __restrict__ partial, const long long* __restrict__ nbt,
                                                     long long* __restrict__ nbt_copy) {
  __shared__ double red[2][4];
  const Bn2dWhere w = bn2d_where(g);
  if (!BWD && nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt_copy = *nbt;
  Chunk<F, V> xv;
  xv.load(x + w.off, w.len);
  double a = 0.0, b = 0.0;
  if constexpr (!BWD) {
    // (elements past the chunk's end were loaded as zeros: they add nothing)
#pragma unroll
    for (int u = 0; u < Chunk<F, V>::U; ++u)
#pragma unroll
      for (int i = 0; i < V; ++i) { const double d = xv.v[u][i]; a += d; b += d * d; }
  } else {
    Chunk<F, V> gv;
    gv.load(dz + w.off, w.len);   // zeros past the end: dy = 0 there
    const float mu = mean[w.ch], is = invstd[w.ch], ga = F::par_load(gamma, w.ch, pd, 1.f), be = F::par_load(beta, w.ch, pd, 0.f);
#pragma unroll
    for (int u = 0; u < Chunk<F, V>::U; ++u)
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float xhat;
        const float y = bn2d_act(xv.v[u][i], mu, is, ga, be, relu, &xhat);
        const float dy = bn2d_masked<F>(y, gv.v[u][i], relu);
        a += dy; b += static_cast<double>(dy) * xhat;
      }
  }
  bn2d_block_sum(a, b, red);
  if (threadIdx.x == 0) {
    double* p = partial + (static_cast<long long>(w.ch) * g.parts + w.part) * 2;
    p[0] = a; p[1] = b;
  }
}

struct Bn2dRun {   // running statistics in the parameters' format
  void* running_mean; void* running_var; long long* num_batches_tracked;
};

// FOLD: batch statistics from the partials (training); otherwise mean / invstd are read from memory (eval mode).
template <class F, int V, bool FOLD>
__global__ __launch_bounds__(256) void bn2d_apply_fwd_k(const typename F::elem* __restrict__ x, Bn2dGeom g, const double* __restrict__ partial,
                                                        const long long* __restrict__ nbt_copy, float* __restrict__ mean,
                                                        float* __restrict__ invstd, Bn2dRun run, float eps, float momentum,
                                                        const void* __restrict__ gamma, const void* __restrict__ beta, int pd, int relu,
                                                        typename F::elem* __restrict__ y) {
  __shared__ double red[2][4];
  __shared__ float sh_stat[2];
  const Bn2dWhere w = bn2d_where(g);
  Chunk<F, V> xv;
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
          const double rm = F::par_load(run.running_mean, w.ch, pd, 0.f), rv = F::par_load(run.running_var, w.ch, pd, 0.f);
          F::par_store(run.running_mean, w.ch, pd, (1.0 - f) * rm + f * m);
          F::par_store(run.running_var, w.ch, pd, (1.0 - f) * rv + f * unbiased);
          if (w.ch == 0 && run.num_batches_tracked) *run.num_batches_tracked = seen + 1;
        }
      }
    }
    __syncthreads();
    mu = sh_stat[0]; is = sh_stat[1];
  } else {
    mu = mean[w.ch]; is = invstd[w.ch];
  }
  const float ga = F::par_load(gamma, w.ch, pd, 1.f), be = F::par_load(beta, w.ch, pd, 0.f);
#pragma unroll
  for (int u = 0; u < Chunk<F, V>::U; ++u)
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float xhat;
      xv.v[u][i] = bn2d_act(xv.v[u][i], mu, is, ga, be, relu, &xhat);
    }
  xv.store(y + w.off, w.len);
}

template <class F, int V>
__global__ __launch_bounds__(256) void bn2d_apply_bwd_k(const typename F::elem* __restrict__ x, const typename F::elem* __restrict__ dz, Bn2dGeom g,
                                                        const double* __restrict__ partial, const float* __restrict__ mean,
                                                        const float* __restrict__ invstd, const void* __restrict__ gamma,
                                                        const void* __restrict__ beta, int pd, int relu, int batch_stats,
                                                        void* __restrict__ dgamma, void* __restrict__ dbeta, typename F::elem* __restrict__ dx) {
  __shared__ double red[2][4];
  __shared__ float sh_coef[2];
  const Bn2dWhere w = bn2d_where(g);
  Chunk<F, V> xv, gv;
  xv.load(x + w.off, w.len);
  gv.load(dz + w.off, w.len);
  double a, b;
  bn2d_fold(partial, g, w.ch, red, &a, &b);
  if (threadIdx.x == 0) {
    if (w.first) { F::par_store(dbeta, w.ch, pd, a); F::par_store(dgamma, w.ch, pd, b); }
    sh_coef[0] = batch_stats ? static_cast<float>(a / g.count) : 0.f;
    sh_coef[1] = batch_stats ? static_cast<float>(b / g.count) : 0.f;
  }
  __syncthreads();
  const float c1 = sh_coef[0], c2 = sh_coef[1];
  const float mu = mean[w.ch], is = invstd[w.ch], ga = F::par_load(gamma, w.ch, pd, 1.f), be = F::par_load(beta, w.ch, pd, 0.f);
#pragma unroll
  for (int u = 0; u < Chunk<F, V>::U; ++u)
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float xhat;
      const float y = bn2d_act(xv.v[u][i], mu, is, ga, be, relu, &xhat);
      const float dy = bn2d_masked<F>(y, gv.v[u][i], relu);
      xv.v[u][i] = ga * is * (dy - c1 - xhat * c2);
    }
  xv.store(dx + w.off, w.len);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
// 0, or the reason the shape cannot be launched
const char* bn2d_geom(int64_t n, int c, int64_t hw, Bn2dGeom* g) {
  g->n = n; g->c = c; g->hw = hw;
  g->chunks = ceil_div(hw, kBn2dChunk);
  if (n > INT32_MAX / g->chunks) return "partials per channel";
  g->parts = static_cast<int>(n * g->chunks);
  if (static_cast<int64_t>(g->parts) * c > kBn2dMaxGrid) return "workgroups";
  g->count = static_cast<double>(n) * static_cast<double>(hw);
  return nullptr;
}

struct Bn2dWs {
  double* partial;       // the fp64 partials and the counter copy: nothing of the map's size
  long long* nbt_copy;
};
template <typename C>
Bn2dWs bn2d_ws(C& cv, const Bn2dGeom& g) {
  Bn2dWs w;
  w.partial = cv.template take<double>(static_cast<size_t>(g.parts) * g.c * 2);
  w.nbt_copy = cv.template take<long long>(1);
  return w;
}

struct FwdArgs2d {
  const void* x; Bn2dGeom g; double* partial; const long long* nbt; long long* nbt_copy; float* mean; float* invstd; Bn2dRun run;
  float eps, momentum; const void* gamma; const void* beta; int pd, relu; void* y;
};
template <class F, int V>
void launch_fwd2d(const FwdArgs2d& a, bool fold, hipStream_t stream) {
  using E = typename F::elem;
  const dim3 grid(static_cast<unsigned>(static_cast<int64_t>(a.g.parts) * a.g.c)), block(256);
  const E* x = static_cast<const E*>(a.x);
  if (fold) {
    hipLaunchKernelGGL((bn2d_reduce_k<F, V, false>), grid, block, 0, stream, x, nullptr, a.g, nullptr, nullptr, nullptr, nullptr, 0, 0, a.partial,
                       a.nbt, a.nbt_copy);
    hipLaunchKernelGGL((bn2d_apply_fwd_k<F, V, true>), grid, block, 0, stream, x, a.g, a.partial, a.nbt_copy, a.mean, a.invstd, a.run, a.eps,
                       a.momentum, a.gamma, a.beta, a.pd, a.relu, static_cast<E*>(a.y));
  } else {
    hipLaunchKernelGGL((bn2d_apply_fwd_k<F, V, false>), grid, block, 0, stream, x, a.g, nullptr, nullptr, a.mean, a.invstd, a.run, a.eps,
                       a.momentum, a.gamma, a.beta, a.pd, a.relu, static_cast<E*>(a.y));
  }
}

struct BwdArgs2d {
  const void* x; const void* dz; Bn2dGeom g; double* partial; const float* mean; const float* invstd; const void* gamma; const void* beta;
  int pd, relu, batch_stats; void* dgamma; void* dbeta; void* dx;
};
template <class F, int V>
void launch_bwd2d(const BwdArgs2d& a, hipStream_t stream) {
  using E = typename F::elem;
  const dim3 grid(static_cast<unsigned>(static_cast<int64_t>(a.g.parts) * a.g.c)), block(256);
  const E* x = static_cast<const E*>(a.x);
  const E* dz = static_cast<const E*>(a.dz);
  hipLaunchKernelGGL((bn2d_reduce_k<F, V, true>), grid, block, 0, stream, x, dz, a.g, a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu, a.partial,
                     nullptr, nullptr);
  hipLaunchKernelGGL((bn2d_apply_bwd_k<F, V>), grid, block, 0, stream, x, dz, a.g, a.partial, a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu,
                     a.batch_stats, a.dgamma, a.dbeta, static_cast<E*>(a.dx));
}

// fn(format, width) for the call's format (dtype 0: fp32) at the vector width, or at 1 where hw or a map's address does not allow it
template <class Fn>
void bn2d_dispatch(int dtype, int64_t hw, bool aligned, Fn fn) {
  auto width = [&](auto f) {
    constexpr int kVec = decltype(f)::kVec;
    if (aligned && hw % kVec == 0) fn(f, std::integral_constant<int, kVec>{});
    else fn(f, std::integral_constant<int, 1>{});
  };
  if (dtype == 0) width(F32{});
  else if (dtype == FV2P_DT_F16) width(Fmt16<H16>{});
  else width(Fmt16<B16>{});
}

// The entry points come in pairs: fp32 (h = false: no dtype arguments) and float16 / bfloat16 (`_h`).
int bn2d_formats(const char* who, bool h, int dtype, int param_dtype) {
  if (!h) return 0;
  FV2P_DT16_OK(who, dtype);
  FV2P_REQUIRE(param_dtype == 0 || param_dtype == dtype, FV2P_EINVAL, "%s: param_dtype %d is neither 0 (fp32) nor the call's dtype %d", who,
               param_dtype, dtype);
  return 0;
}

size_t bn2d_ws_bytes(int64_t n, int c, int64_t hw) {
  Bn2dGeom g;
  if (n < 1 || c < 1 || hw < 1 || bn2d_geom(n, c, hw, &g)) return 0;
  Sizer s;
  bn2d_ws(s, g);
  return s.bytes();
}

int bn2d_forward(bool h, const void* x, int64_t n, int c, int64_t hw, float eps, float momentum, const void* gamma, const void* beta, int relu,
                 void* running_mean, void* running_var, int64_t* num_batches_tracked, float* mean, float* invstd, void* y, int dtype,
                 int param_dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const char* who = h ? "batchnorm2d_forward_h" : "batchnorm2d_forward";
  if (const int rc = bn2d_formats(who, h, dtype, param_dtype)) return rc;
  FV2P_REQUIRE(n >= 1 && c >= 1 && hw >= 1, FV2P_EINVAL, "%s: n=%lld c=%d hw=%lld", who, static_cast<long long>(n), c, static_cast<long long>(hw));
  FV2P_REQUIRE(x && y && mean && invstd && ws, FV2P_EINVAL, "%s: null pointer", who);
  FV2P_REQUIRE((running_mean == nullptr) == (running_var == nullptr), FV2P_EINVAL, "%s: running_mean and running_var come together", who);
  Bn2dGeom g;
  const char* why = bn2d_geom(n, c, hw, &g);
  FV2P_REQUIRE(!why, FV2P_ELIMIT, "%s: too many %s (n=%lld c=%d hw=%lld)", who, why, static_cast<long long>(n), c, static_cast<long long>(hw));
  FV2P_REQUIRE(ws_bytes >= bn2d_ws_bytes(n, c, hw), FV2P_EWORKSPACE, "%s: workspace %lld < %lld", who, static_cast<long long>(ws_bytes),
               static_cast<long long>(bn2d_ws_bytes(n, c, hw)));
  Carver cv(ws, ws_bytes);
  const Bn2dWs w = bn2d_ws(cv, g);
  const FwdArgs2d a{x, g, w.partial, reinterpret_cast<const long long*>(running_mean ? num_batches_tracked : nullptr), w.nbt_copy, mean, invstd,
                    Bn2dRun{running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked)}, eps, momentum, gamma, beta,
                    param_dtype != 0, relu, y};
  bn2d_dispatch(dtype, hw, aligned16(x) && aligned16(y), [&](auto f, auto v) { launch_fwd2d<decltype(f), decltype(v)::value>(a, true, stream); });
  FV2P_LAUNCH_CHECK();
  return 0;
}

int bn2d_apply(bool h, const void* x, int64_t n, int c, int64_t hw, const float* mean, const float* invstd, const void* gamma, const void* beta,
               int relu, void* y, int dtype, int param_dtype, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const char* who = h ? "batchnorm2d_apply_h" : "batchnorm2d_apply";
  if (const int rc = bn2d_formats(who, h, dtype, param_dtype)) return rc;
  FV2P_REQUIRE(n >= 0 && c >= 1 && hw >= 0, FV2P_EINVAL, "%s: n=%lld c=%d hw=%lld", who, static_cast<long long>(n), c, static_cast<long long>(hw));
  if (n == 0 || hw == 0) return 0;
  FV2P_REQUIRE(x && y && mean && invstd, FV2P_EINVAL, "%s: null pointer", who);
  Bn2dGeom g;
  const char* why = bn2d_geom(n, c, hw, &g);
  FV2P_REQUIRE(!why, FV2P_ELIMIT, "%s: too many %s (n=%lld c=%d hw=%lld)", who, why, static_cast<long long>(n), c, static_cast<long long>(hw));
  const FwdArgs2d a{x, g, nullptr, nullptr, nullptr, const_cast<float*>(mean), const_cast<float*>(invstd), Bn2dRun{nullptr, nullptr, nullptr},
                    0.f, 0.f, gamma, beta, param_dtype != 0, relu, y};
  bn2d_dispatch(dtype, hw, aligned16(x) && aligned16(y), [&](auto f, auto v) { launch_fwd2d<decltype(f), decltype(v)::value>(a, false, stream); });
  FV2P_LAUNCH_CHECK();
  return 0;
}

int bn2d_backward(bool h, const void* x, const void* dz, int64_t n, int c, int64_t hw, const float* mean, const float* invstd, const void* gamma,
                  const void* beta, int relu, int batch_stats, void* dx, void* dgamma, void* dbeta, int dtype, int param_dtype, void* ws,
                  size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const char* who = h ? "batchnorm2d_backward_h" : "batchnorm2d_backward";
  if (const int rc = bn2d_formats(who, h, dtype, param_dtype)) return rc;
  FV2P_REQUIRE(n >= 1 && c >= 1 && hw >= 1, FV2P_EINVAL, "%s: n=%lld c=%d hw=%lld", who, static_cast<long long>(n), c, static_cast<long long>(hw));
  FV2P_REQUIRE(x && dz && mean && invstd && dx && dgamma && dbeta && ws, FV2P_EINVAL, "%s: null pointer", who);
  Bn2dGeom g;
  const char* why = bn2d_geom(n, c, hw, &g);
  FV2P_REQUIRE(!why, FV2P_ELIMIT, "%s: too many %s (n=%lld c=%d hw=%lld)", who, why, static_cast<long long>(n), c, static_cast<long long>(hw));
  FV2P_REQUIRE(ws_bytes >= bn2d_ws_bytes(n, c, hw), FV2P_EWORKSPACE, "%s: workspace %lld < %lld", who, static_cast<long long>(ws_bytes),
               static_cast<long long>(bn2d_ws_bytes(n, c, hw)));
  Carver cv(ws, ws_bytes);
  const Bn2dWs w = bn2d_ws(cv, g);
  const BwdArgs2d a{x, dz, g, w.partial, mean, invstd, gamma, beta, param_dtype != 0, relu, batch_stats, dgamma, dbeta, dx};
  bn2d_dispatch(dtype, hw, aligned16(x) && aligned16(dz) && aligned16(dx),
                [&](auto f, auto v) { launch_bwd2d<decltype(f), decltype(v)::value>(a, stream); });
  FV2P_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace fv2p

using namespace fv2p;

extern "C" size_t fv2p_batchnorm2d_ws_bytes(int64_t n, int c, int64_t hw) { return bn2d_ws_bytes(n, c, hw); }
extern "C" size_t fv2p_batchnorm2d_h_ws_bytes(int64_t n, int c, int64_t hw) { return bn2d_ws_bytes(n, c, hw); }

extern "C" int fv2p_batchnorm2d_forward(const float* x, int64_t n, int c, int64_t hw, float eps, float momentum, const float* gamma,
                                        const float* beta, int relu, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                        float* mean, float* invstd, float* y, void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  return bn2d_forward(false, x, n, c, hw, eps, momentum, gamma, beta, relu, running_mean, running_var, num_batches_tracked, mean, invstd, y, 0, 0, ws,
                      ws_bytes, stream);
}
extern "C" int fv2p_batchnorm2d_forward_h(const void* x, int64_t n, int c, int64_t hw, float eps, float momentum, const void* gamma,
                                          const void* beta, int relu, void* running_mean, void* running_var, int64_t* num_batches_tracked,
                                          float* mean, float* invstd, void* y, int dtype, int param_dtype, void* ws, size_t ws_bytes,
                                          fv2p_stream_t stream) {
  return bn2d_forward(true, x, n, c, hw, eps, momentum, gamma, beta, relu, running_mean, running_var, num_batches_tracked, mean, invstd, y, dtype,
                      param_dtype, ws, ws_bytes, stream);
}

extern "C" int fv2p_batchnorm2d_apply(const float* x, int64_t n, int c, int64_t hw, const float* mean, const float* invstd, const float* gamma,
                                      const float* beta, int relu, float* y, fv2p_stream_t stream) {
  return bn2d_apply(false, x, n, c, hw, mean, invstd, gamma, beta, relu, y, 0, 0, stream);
}
extern "C" int fv2p_batchnorm2d_apply_h(const void* x, int64_t n, int c, int64_t hw, const float* mean, const float* invstd, const void* gamma,
                                        const void* beta, int relu, void* y, int dtype, int param_dtype, fv2p_stream_t stream) {
  return bn2d_apply(true, x, n, c, hw, mean, invstd, gamma, beta, relu, y, dtype, param_dtype, stream);
}

extern "C" int fv2p_batchnorm2d_backward(const float* x, const float* dz, int64_t n, int c, int64_t hw, const float* mean, const float* invstd,
                                         const float* gamma, const float* beta, int relu, int batch_stats, float* dx, float* dgamma,
                                         float* dbeta, void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  return bn2d_backward(false, x, dz, n, c, hw, mean, invstd, gamma, beta, relu, batch_stats, dx, dgamma, dbeta, 0, 0, ws, ws_bytes, stream);
}
extern "C" int fv2p_batchnorm2d_backward_h(const void* x, const void* dz, int64_t n, int c, int64_t hw, const float* mean, const float* invstd,
                                           const void* gamma, const void* beta, int relu, int batch_stats, void* dx, void* dgamma, void* dbeta,
                                           int dtype, int param_dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  return bn2d_backward(true, x, dz, n, c, hw, mean, invstd, gamma, beta, relu, batch_stats, dx, dgamma, dbeta, dtype, param_dtype, ws, ws_bytes, stream);
}
