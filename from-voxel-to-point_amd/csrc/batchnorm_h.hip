// BatchNorm1d (+ residual, + ReLU) over sparse-tensor features [N, C] stored in 16 bits (float16 / bfloat16) - the layers between two
// convs of csrc/sparse_conv_h.hip, so that a backbone block stays on 16-bit storage forward and backward.
//
// The two-launch form of batchnorm.hip, nothing else:
//   forward : bn_reduce_h_k<FWD>  per-channel sum / sum of squares of the widened elements in fp64, one partial per workgroup (<= 64);
//             bn_apply_fwd_h_k    every workgroup folds the partials in the same fixed order (fold_chunk), workgroup 0 also stores
//                                 mean / invstd (always fp32) and moves the running statistics;
//                                 y = round16(relu?((x - mean) * invstd * gamma + beta [+ residual])), all in fp32, ONE rounding
//   backward: bn_reduce_h_k<BWD>  dz = dy * [y > 0] (mask recomputed from x, or read from mask_y);  sum dz, sum dz * xhat
//             bn_apply_bwd_h_k    folds to dbeta, dgamma, c1, c2;  dx = round16(gamma * invstd * (dz - c1 - xhat * c2))
// The kernel boundary is the only synchronisation: no float atomics, no grid barrier, no last-workgroup protocol (the one-launch and
// in-conv finalisation forms of the fp32 file are not ported).  Results are bit-identical from run to run.
// Rows travel as 16-byte accesses of 8 elements per lane when c % 8 == 0 and every tensor is 16-byte aligned (c <= 1024), element by
// element otherwise (c <= 256).  Parameters (gamma, beta, running statistics, dgamma, dbeta) are fp32 or the call's 16-bit format
// (`pd`): widened on read; written from the fp64 value with a single rounding.
#include "common.hpp"
#include "bn_fold.hpp"
#include "dt16.hpp"

namespace fv2p {
namespace {

constexpr int kBnMaxC = 1024;
constexpr int kBnPartials = 64;

// partial: [nblk][2][c] doubles, as bn_reduce_k
template <class T, int V, bool BWD>
__global__ __launch_bounds__(256) void bn_reduce_h_k(const u16* __restrict__ x, const u16* __restrict__ dy, BnGeom g,
                                                     const float* __restrict__ mean, const float* __restrict__ invstd,
                                                     const void* __restrict__ gamma, const void* __restrict__ beta, int pd, int relu,
                                                     double* __restrict__ partial, const u16* __restrict__ mask_y) {
  __shared__ double red[2][256 * V];
  const int tid = threadIdx.x;
  const int rl = tid / g.tcols, cq = tid % g.tcols;
  const int col = cq * V;
  const bool live = rl < g.rpp && col < g.c;
  double s1[V], s2[V];
#pragma unroll
  for (int i = 0; i < V; ++i) s1[i] = s2[i] = 0.0;
  if (live) {
    float m[V] = {}, is[V] = {}, ga[V] = {}, be[V] = {};
    if (BWD) {
#pragma unroll
      for (int i = 0; i < V; ++i) {
        m[i] = mean[col + i]; is[i] = invstd[col + i];
        ga[i] = par_load<T>(gamma, col + i, pd, 1.f); be[i] = par_load<T>(beta, col + i, pd, 0.f);
      }
    }
    const long long r0 = static_cast<long long>(blockIdx.x) * g.rows_per_block;
    const long long r1 = min(r0 + g.rows_per_block, g.n);
    constexpr int U = 4;   // rows in flight per thread (16 bytes each per tensor)
    auto accumulate = [&](const Row16<T, V>& xv, const Row16<T, V>& gv, const Row16<T, V>& mv) {
      if (!BWD) {
#pragma unroll
        for (int i = 0; i < V; ++i) { const double d = xv.v[i]; s1[i] += d; s2[i] += d * d; }
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const float xhat = (xv.v[i] - m[i]) * is[i];
          const float y = mask_y ? mv.v[i] : xhat * ga[i] + be[i];
          const float dz = (relu && !(y > 0.f)) ? 0.f : gv.v[i];
          s1[i] += dz; s2[i] += static_cast<double>(dz) * xhat;
        }
      }
    };
    long long r = r0 + rl;
    for (; r + static_cast<long long>(U - 1) * g.rpp < r1; r += static_cast<long long>(U) * g.rpp) {
      Row16<T, V> xv[U], gv[U], mv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long at = (r + static_cast<long long>(u) * g.rpp) * g.c + col;
        xv[u].load(x + at);
        if (BWD) gv[u].load(dy + at);
        if (BWD && mask_y) mv[u].load(mask_y + at);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) accumulate(xv[u], gv[u], mv[u]);
    }
    for (; r < r1; r += g.rpp) {
      Row16<T, V> xv, gv, mv;
      xv.load(x + r * g.c + col);
      if (BWD) gv.load(dy + r * g.c + col);
      if (BWD && mask_y) mv.load(mask_y + r * g.c + col);
      accumulate(xv, gv, mv);
    }
  }
  // fold the row lanes: red[.][rl * cpad + col]
  if (rl < g.rpp) {
#pragma unroll
    for (int i = 0; i < V; ++i) { red[0][(rl * g.tcols + cq) * V + i] = s1[i]; red[1][(rl * g.tcols + cq) * V + i] = s2[i]; }
  }
  __syncthreads();
  const int cpad = g.tcols * V;
  for (int e = tid; e < cpad; e += 256) {
    double a = 0.0, b = 0.0;
    for (int q = 0; q < g.rpp; ++q) { a += red[0][q * cpad + e]; b += red[1][q * cpad + e]; }
    if (e < g.c) {
      partial[(static_cast<long long>(blockIdx.x) * 2 + 0) * g.c + e] = a;
      partial[(static_cast<long long>(blockIdx.x) * 2 + 1) * g.c + e] = b;
    }
  }
}

struct BnRun16 {   // running statistics in the parameters' format (pd: 16-bit) - the fp32 ones go through BnFwdFin
  void* running_mean; void* running_var;
};

// FOLD: batch statistics from the partials (training); otherwise mean / invstd are read from memory (eval mode)
template <class T, int V, bool FOLD>
__global__ __launch_bounds__(256) void bn_apply_fwd_h_k(const u16* __restrict__ x, long long units, BnGeom g, const double* __restrict__ partial,
                                                        BnFwdFin ff, BnRun16 run16, const void* __restrict__ gamma, const void* __restrict__ beta,
                                                        int pd, int relu, u16* __restrict__ y, const u16* __restrict__ residual) {
  __shared__ double red[2][256];
  __shared__ float sh_mean[kBnMaxC], sh_is[kBnMaxC], sh_gamma[kBnMaxC], sh_beta[kBnMaxC];
  const int tid = threadIdx.x, c = g.c;
  const int cfold = c < 256 ? c : 256;
  for (int e0 = 0; e0 < c; e0 += cfold) {
    const int e = e0 + tid;
    float mu_f = 0.f, is_f = 0.f;
    if (FOLD) {
      double a, b;
      fold_chunk<false>(g.nblk, c, partial, e0, cfold, red, &a, &b);
      if (tid < cfold && e < c) {
        bn_fwd_channel(a, b, g.n, ff, e, blockIdx.x == 0, &mu_f, &is_f);   // (ff.running_* are null when the buffers are 16-bit)
        if (blockIdx.x == 0 && run16.running_mean) {
          // the same update on the widened old values, from the fp64 statistics, rounded once to 16 bits
          const double n = static_cast<double>(g.n);
          const double mu = a / n;
          double var = b / n - mu * mu;
          if (var < 0.0) var = 0.0;
          double f = ff.momentum;
          if (ff.momentum < 0.f) f = 1.0 / static_cast<double>(ff.num_batches_tracked ? (*ff.num_batches_tracked + 1) : 1);
          const double unbiased = g.n > 1 ? var * n / (n - 1.0) : var;
          const double rm = T::widen(static_cast<const u16*>(run16.running_mean)[e]);
          const double rv = T::widen(static_cast<const u16*>(run16.running_var)[e]);
          par_store<T>(run16.running_mean, e, 1, (1.0 - f) * rm + f * mu);
          par_store<T>(run16.running_var, e, 1, (1.0 - f) * rv + f * unbiased);
        }
      }
    } else {
      mu_f = (tid < cfold && e < c) ? ff.mean[e] : 0.f;
      is_f = (tid < cfold && e < c) ? ff.invstd[e] : 0.f;
    }
    if (tid < cfold && e < c) {
      sh_mean[e] = mu_f;
      sh_is[e] = is_f;
      sh_gamma[e] = par_load<T>(gamma, e, pd, 1.f);
      sh_beta[e] = par_load<T>(beta, e, pd, 0.f);
    }
  }
  // momentum=None: every channel above read *num_batches_tracked; the bump must not overtake a channel of another wave
  __syncthreads();
  if (FOLD && blockIdx.x == 0 && tid == 0 && (ff.running_mean || run16.running_mean) && ff.num_batches_tracked) *ff.num_batches_tracked += 1;
  const int cv = c / V;
  for (long long u = static_cast<long long>(blockIdx.x) * 256 + tid; u < units; u += static_cast<long long>(gridDim.x) * 256) {
    const int col = static_cast<int>(u % cv) * V;
    Row16<T, V> xv, rv, o;
    xv.load(x + u * V);
    if (residual) rv.load(residual + u * V);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float xhat = (xv.v[i] - sh_mean[col + i]) * sh_is[col + i];
      float t = xhat * sh_gamma[col + i] + sh_beta[col + i];
      if (residual) t = t + rv.v[i];
      o.v[i] = (relu && t <= 0.f) ? 0.f : t;  // NaN passes through, like torch.relu
    }
    o.store(y + u * V);
  }
}

template <class T, int V>
__global__ __launch_bounds__(256) void bn_apply_bwd_h_k(const u16* __restrict__ x, const u16* __restrict__ dy, long long units, BnGeom g,
                                                        const double* __restrict__ partial, const float* __restrict__ mean,
                                                        const float* __restrict__ invstd, const void* __restrict__ gamma,
                                                        const void* __restrict__ beta, int pd, int relu, int batch_stats, void* __restrict__ dgamma,
                                                        void* __restrict__ dbeta, u16* __restrict__ dx, const u16* __restrict__ mask_y,
                                                        u16* __restrict__ dz_out) {
  __shared__ double red[2][256];
  __shared__ float sh_mean[kBnMaxC], sh_is[kBnMaxC], sh_gamma[kBnMaxC], sh_beta[kBnMaxC], sh_c1[kBnMaxC], sh_c2[kBnMaxC];
  const int tid = threadIdx.x, c = g.c;
  const int cfold = c < 256 ? c : 256;
  for (int e0 = 0; e0 < c; e0 += cfold) {
    const int e = e0 + tid;
    double a, b;
    fold_chunk<false>(g.nblk, c, partial, e0, cfold, red, &a, &b);
    if (tid < cfold && e < c) {
      const double n = static_cast<double>(g.n);
      if (blockIdx.x == 0) {
        par_store<T>(dbeta, e, pd, a);
        par_store<T>(dgamma, e, pd, b);
      }
      sh_c1[e] = batch_stats ? static_cast<float>(a / n) : 0.f;
      sh_c2[e] = batch_stats ? static_cast<float>(b / n) : 0.f;
      sh_mean[e] = mean[e];
      sh_is[e] = invstd[e];
      sh_gamma[e] = par_load<T>(gamma, e, pd, 1.f);
      sh_beta[e] = par_load<T>(beta, e, pd, 0.f);
    }
  }
  __syncthreads();
  const int cv = c / V;
  for (long long u = static_cast<long long>(blockIdx.x) * 256 + tid; u < units; u += static_cast<long long>(gridDim.x) * 256) {
    const int col = static_cast<int>(u % cv) * V;
    Row16<T, V> xv, gv, mv, o, z;
    xv.load(x + u * V);
    gv.load(dy + u * V);
    if (mask_y) mv.load(mask_y + u * V);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float is = sh_is[col + i], ga = sh_gamma[col + i];
      const float xhat = (xv.v[i] - sh_mean[col + i]) * is;
      const float t = mask_y ? mv.v[i] : xhat * ga + sh_beta[col + i];
      const float dz = (relu && !(t > 0.f)) ? 0.f : gv.v[i];
      z.v[i] = dz;
      o.v[i] = ga * is * (dz - sh_c1[col + i] - xhat * sh_c2[col + i]);
    }
    o.store(dx + u * V);
    if (dz_out) z.store(dz_out + u * V);   // dz is dy or 0: stored exactly
  }
}

int bn_geom_h(int64_t n, int c, bool vec, BnGeom* g) {
  const int v = vec ? 8 : 1;
  g->n = n; g->c = c;
  g->tcols = static_cast<int>(ceil_div(c, v));
  if (g->tcols > 256 || c > kBnMaxC) return -1;
  g->rpp = 256 / g->tcols;
  // >= 8 rows per row lane per workgroup, at most kBnPartials workgroups (every apply workgroup re-folds the partials)
  int64_t nblk = ceil_div(n, static_cast<int64_t>(g->rpp) * 8);
  if (nblk > kBnPartials) nblk = kBnPartials;
  if (nblk < 1) nblk = 1;
  g->rows_per_block = ceil_div(n, nblk);
  g->nblk = static_cast<int>(ceil_div(n, g->rows_per_block));
  return 0;
}

unsigned apply_blocks_h(long long units) {
  // grid-stride, ~4 units per thread, at most 2 workgroups per CU worth of fold prologues
  const int64_t b = ceil_div(units, 256 * 4);
  return static_cast<unsigned>(b > 512 ? 512 : (b < 1 ? 1 : b));
}

struct FwdArgs {
  const u16* x; int64_t n; int c; BnGeom g; bool vec;
  double* partial; BnFwdFin ff; BnRun16 run16; const void* gamma; const void* beta; int pd; int relu; u16* y; const u16* residual;
};
template <class T, int V>
void launch_fwd(const FwdArgs& a, bool fold, hipStream_t stream) {
  const long long units = a.n * a.c / V;
  const unsigned blocks = apply_blocks_h(units);
  if (fold) {
    hipLaunchKernelGGL((bn_reduce_h_k<T, V, false>), dim3(a.g.nblk), dim3(256), 0, stream, a.x, nullptr, a.g, nullptr, nullptr, nullptr, nullptr, 0, 0,
                       a.partial, nullptr);
    hipLaunchKernelGGL((bn_apply_fwd_h_k<T, V, true>), dim3(blocks), dim3(256), 0, stream, a.x, units, a.g, a.partial, a.ff, a.run16, a.gamma, a.beta,
                       a.pd, a.relu, a.y, a.residual);
  } else {
    hipLaunchKernelGGL((bn_apply_fwd_h_k<T, V, false>), dim3(blocks), dim3(256), 0, stream, a.x, units, a.g, nullptr, a.ff, a.run16, a.gamma, a.beta,
                       a.pd, a.relu, a.y, a.residual);
  }
}
template <class T>
void launch_fwd(const FwdArgs& a, bool fold, hipStream_t stream) {
  if (a.vec) launch_fwd<T, 8>(a, fold, stream);
  else launch_fwd<T, 1>(a, fold, stream);
}

struct BwdArgs {
  const u16* x; const u16* dy; int64_t n; int c; BnGeom g; bool vec;
  double* partial; const float* mean; const float* invstd; const void* gamma; const void* beta; int pd; int relu; int batch_stats;
  void* dgamma; void* dbeta; u16* dx; const u16* mask_y; u16* dz_out;
};
template <class T, int V>
void launch_bwd(const BwdArgs& a, hipStream_t stream) {
  const long long units = a.n * a.c / V;
  hipLaunchKernelGGL((bn_reduce_h_k<T, V, true>), dim3(a.g.nblk), dim3(256), 0, stream, a.x, a.dy, a.g, a.mean, a.invstd, a.gamma, a.beta, a.pd, a.relu,
                     a.partial, a.mask_y);
  hipLaunchKernelGGL((bn_apply_bwd_h_k<T, V>), dim3(apply_blocks_h(units)), dim3(256), 0, stream, a.x, a.dy, units, a.g, a.partial, a.mean, a.invstd,
                     a.gamma, a.beta, a.pd, a.relu, a.batch_stats, a.dgamma, a.dbeta, a.dx, a.mask_y, a.dz_out);
}
template <class T>
void launch_bwd(const BwdArgs& a, hipStream_t stream) {
  if (a.vec) launch_bwd<T, 8>(a, stream);
  else launch_bwd<T, 1>(a, stream);
}

}  // namespace
}  // namespace fv2p

using namespace fv2p;

#define FV2P_BN_H_DTYPES(name)                                                                                                                  \
  FV2P_DT16_OK(name, dtype);                                                                                                                    \
  FV2P_REQUIRE(param_dtype == 0 || param_dtype == dtype, FV2P_EINVAL, name ": param_dtype %d is neither 0 (fp32) nor the call's dtype %d",     \
               param_dtype, dtype)

extern "C" size_t fv2p_batchnorm_h_ws_bytes(int64_t n, int c) {
  (void)n;
  Sizer s;
  s.take<double>(static_cast<size_t>(kBnPartials) * 2 * (c > 0 ? c : 1));
  return s.bytes();
}

extern "C" int fv2p_batchnorm_forward_h(const void* x, int64_t n, int c, float eps, float momentum, const void* gamma, const void* beta, int relu,
                                        const void* residual, void* running_mean, void* running_var, int64_t* num_batches_tracked, float* mean,
                                        float* invstd, void* y, int dtype, int param_dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FV2P_BN_H_DTYPES("batchnorm_forward_h");
  FV2P_REQUIRE(n >= 0 && c >= 1, FV2P_EINVAL, "batchnorm_forward_h: n=%lld c=%d", static_cast<long long>(n), c);
  if (n == 0) return 0;
  FV2P_REQUIRE(x && y && mean && invstd && ws, FV2P_EINVAL, "batchnorm_forward_h: null pointer");
  FV2P_REQUIRE((running_mean == nullptr) == (running_var == nullptr), FV2P_EINVAL, "batchnorm_forward_h: running_mean and running_var come together");
  FV2P_REQUIRE(ws_bytes >= fv2p_batchnorm_h_ws_bytes(n, c), FV2P_EWORKSPACE, "batchnorm_forward_h: workspace %lld < %lld",
               static_cast<long long>(ws_bytes), static_cast<long long>(fv2p_batchnorm_h_ws_bytes(n, c)));
  FwdArgs a;
  a.vec = (c % 8 == 0) && aligned16(x) && aligned16(y) && (!residual || aligned16(residual));
  FV2P_REQUIRE(bn_geom_h(n, c, a.vec, &a.g) == 0, FV2P_ELIMIT, "batchnorm_h: c=%d exceeds %d", c, a.vec ? kBnMaxC : 256);
  Carver cv(ws, ws_bytes);
  a.partial = cv.take<double>(static_cast<size_t>(kBnPartials) * 2 * c);
  const bool run32 = running_mean && param_dtype == 0;
  a.ff = BnFwdFin{mean, invstd, run32 ? static_cast<float*>(running_mean) : nullptr, run32 ? static_cast<float*>(running_var) : nullptr,
                  reinterpret_cast<long long*>(num_batches_tracked), momentum, eps};
  a.run16 = (running_mean && param_dtype != 0) ? BnRun16{running_mean, running_var} : BnRun16{nullptr, nullptr};
  a.x = static_cast<const u16*>(x); a.n = n; a.c = c; a.gamma = gamma; a.beta = beta; a.pd = param_dtype != 0; a.relu = relu;
  a.y = static_cast<u16*>(y); a.residual = static_cast<const u16*>(residual);
  if (dtype == FV2P_DT_F16) launch_fwd<H16>(a, true, stream);
  else launch_fwd<B16>(a, true, stream);
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" int fv2p_batchnorm_apply_h(const void* x, int64_t n, int c, const float* mean, const float* invstd, const void* gamma, const void* beta,
                                      int relu, const void* residual, void* y, int dtype, int param_dtype, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FV2P_BN_H_DTYPES("batchnorm_apply_h");
  FV2P_REQUIRE(n >= 0 && c >= 1, FV2P_EINVAL, "batchnorm_apply_h: n=%lld c=%d", static_cast<long long>(n), c);
  if (n == 0) return 0;
  FV2P_REQUIRE(x && y && mean && invstd, FV2P_EINVAL, "batchnorm_apply_h: null pointer");
  FwdArgs a;
  a.vec = (c % 8 == 0) && aligned16(x) && aligned16(y) && (!residual || aligned16(residual));
  FV2P_REQUIRE(bn_geom_h(n, c, a.vec, &a.g) == 0, FV2P_ELIMIT, "batchnorm_h: c=%d exceeds %d", c, a.vec ? kBnMaxC : 256);
  a.partial = nullptr;
  a.ff = BnFwdFin{const_cast<float*>(mean), const_cast<float*>(invstd), nullptr, nullptr, nullptr, 0.f, 0.f};
  a.run16 = BnRun16{nullptr, nullptr};
  a.x = static_cast<const u16*>(x); a.n = n; a.c = c; a.gamma = gamma; a.beta = beta; a.pd = param_dtype != 0; a.relu = relu;
  a.y = static_cast<u16*>(y); a.residual = static_cast<const u16*>(residual);
  if (dtype == FV2P_DT_F16) launch_fwd<H16>(a, false, stream);
  else launch_fwd<B16>(a, false, stream);
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" int fv2p_batchnorm_backward_h(const void* x, const void* dy, int64_t n, int c, const float* mean, const float* invstd, const void* gamma,
                                         const void* beta, int relu, int batch_stats, const void* mask_y, void* dx, void* dz_out, void* dgamma,
                                         void* dbeta, int dtype, int param_dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FV2P_BN_H_DTYPES("batchnorm_backward_h");
  FV2P_REQUIRE(n >= 0 && c >= 1, FV2P_EINVAL, "batchnorm_backward_h: n=%lld c=%d", static_cast<long long>(n), c);
  if (n == 0) return 0;
  FV2P_REQUIRE(x && dy && mean && invstd && dx && dgamma && dbeta && ws, FV2P_EINVAL, "batchnorm_backward_h: null pointer");
  FV2P_REQUIRE(ws_bytes >= fv2p_batchnorm_h_ws_bytes(n, c), FV2P_EWORKSPACE, "batchnorm_backward_h: workspace %lld < %lld",
               static_cast<long long>(ws_bytes), static_cast<long long>(fv2p_batchnorm_h_ws_bytes(n, c)));
  BwdArgs a;
  a.vec = (c % 8 == 0) && aligned16(x) && aligned16(dy) && aligned16(dx) && (!mask_y || aligned16(mask_y)) && (!dz_out || aligned16(dz_out));
  FV2P_REQUIRE(bn_geom_h(n, c, a.vec, &a.g) == 0, FV2P_ELIMIT, "batchnorm_h: c=%d exceeds %d", c, a.vec ? kBnMaxC : 256);
  Carver cv(ws, ws_bytes);
  a.partial = cv.take<double>(static_cast<size_t>(kBnPartials) * 2 * c);
  a.x = static_cast<const u16*>(x); a.dy = static_cast<const u16*>(dy); a.n = n; a.c = c;
  a.mean = mean; a.invstd = invstd; a.gamma = gamma; a.beta = beta; a.pd = param_dtype != 0; a.relu = relu; a.batch_stats = batch_stats;
  a.dgamma = dgamma; a.dbeta = dbeta; a.dx = static_cast<u16*>(dx); a.mask_y = static_cast<const u16*>(mask_y); a.dz_out = static_cast<u16*>(dz_out);
  if (dtype == FV2P_DT_F16) launch_bwd<H16>(a, stream);
  else launch_bwd<B16>(a, stream);
  FV2P_LAUNCH_CHECK();
  return 0;
}
