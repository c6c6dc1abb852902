// BatchNorm1d (+ residual, + ReLU) over sparse-tensor features [N, C] in fp32, float16 or bfloat16 - SURVEY §8(f).3.
//
// Every conv of the reference's sparse backbones is followed by BatchNorm1d(eps=1e-3, momentum=0.01) + ReLU
// (pcdet/models/backbones_3d/spconv_backbone.py:8-27 post_act_block, :75 conv_input).  On [N, C] with C = 16..128 torch's
// channels-last BN kernels run 25-30 us per call at N ~ 5e4 (profiles/r01_bench_kernel_stats.csv), i.e. ~0.25 TB/s; here the layer is
// plain coalesced 16-byte streams, two launches forward and two backward:
//   forward : bn_reduce_k<FWD>  per-channel sum / sum of squares in fp64, one partial per workgroup (<= 64 of them);
//             bn_apply_fwd_k    every workgroup folds the partials in the same fixed order (deterministic; the kernel boundary replaces
//                               an agent-scope fence per producer, which on gfx950 writes the whole L2 back: measured 20 us per
//                               launch), workgroup 0 also stores mean / invstd (always fp32) and moves the running statistics; then
//                               y = relu?((x - mean) * invstd * gamma + beta [+ residual]), all in fp32, ONE rounding on the store
//   backward: bn_reduce_k<BWD>  dz = dy * [y > 0] (mask recomputed from x, or read from mask_y);  sum dz, sum dz * xhat
//             bn_apply_bwd_k    folds to dbeta, dgamma, c1, c2;  dx = gamma * invstd * (dz - c1 - xhat * c2)
// The ReLU mask is recomputed from x, so y is not needed by the backward pass.  It is the mask of the UNROUNDED fp32 pre-activation
// (!(t > 0)) in every format; batchnorm2d.hip masks by the stored output, F::stored(t) - a known difference between the two layers.
//
// One source, three storage formats (bn_fmt.hpp: F32, Fmt16<H16>, Fmt16<B16>).  Written once, templated on <F, V, ...>: the row
// reduction (bn_reduce_rows), the two fold-and-finalise prologues (bn_fwd_prologue, bn_bwd_prologue), the two per-element loops
// (bn_fwd_rows, bn_bwd_rows) and, in bn_fold.hpp, the running-statistics update (bn_move_running).  Rows travel as 16-byte accesses of
// F::kVec elements per lane when c % F::kVec == 0 and every tensor is 16-byte aligned (c <= 1024), element by element otherwise
// (c <= 256).  16-bit rows take their parameters (gamma, beta, running statistics, dgamma, dbeta) in fp32 or in the rows' format (`pd`):
// widened on read, written from the fp64 value with a single rounding.
// Routes.  All three formats: the two-launch form above.  fp32 only, so far: the conv-epilogue statistics (`_stats`: the partials are
// the slots a conv launch accumulated; the apply launch clears the other slot buffer), statistics the producing conv finalised
// (`_fin`: BnBwdOut::coef), the one-launch form (bn_one_*: reduce, grid barrier, apply) and the wide form (bn_reduce_fin_k: reduce on
// up to 512 workgroups whose last ones finalise, then a fold-free apply).  What one side alone uses is compiled out of the other.
#include <initializer_list>
#include <type_traits>
#include "common.hpp"
#include "bn_fold.hpp"

namespace fv2p {
namespace {

constexpr int kBnMaxC = 1024;
constexpr int kBnPartials = 64;
static_assert(kStatSlots <= kBnPartials, "the fallback passes write their partials into the statistics slots");

template <class F>
constexpr bool kIs32 = std::is_same<F, F32>::value;

// ---- the row reduction ------------------------------------------------------------------------------------------------------------------
// Per-channel (a, b) sums of this workgroup's rows -> partial[blockIdx.x][2][c] doubles.  Rows are accumulated in row order inside a
// thread, the row lanes folded in order through LDS.  PUBLISH: other workgroups of THIS launch read the partial (stat_publish:
// bn_fold.hpp); otherwise a plain store that the kernel boundary orders.
// mask_y (backward only, the residual form): the ReLU that follows is relu(bn(x) + identity), so its mask is read from the block's
// OUTPUT (mask_y > 0) instead of being recomputed from x.
template <class F, int V, bool BWD, bool PUBLISH>
__device__ __forceinline__ void bn_reduce_rows(const typename F::elem* __restrict__ x, const typename F::elem* __restrict__ dy, const BnGeom& g,
                                               const float* mean, const float* invstd, const void* gamma, const void* beta, int pd, int relu,
                                               const typename F::elem* mask_y, double* partial, double (*red)[256 * V]) {
  using Unit = typename F::template Unit<V>;
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
        ga[i] = F::par_load(gamma, col + i, pd, 1.f); be[i] = F::par_load(beta, col + i, pd, 0.f);
      }
    }
    const long long r0 = static_cast<long long>(blockIdx.x) * g.rows_per_block;
    const long long r1 = min(r0 + g.rows_per_block, g.n);
    // U rows in flight per thread (16 bytes each per tensor): the pass is latency bound (a few MB spread over the whole chip), so the
    // loads of a group are all issued before the first fp64 add
    constexpr int U = F::kRows;
    auto accumulate = [&](const Unit& xv, const Unit& gv, const Unit& mv) {
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
      Unit xv[U], gv[U], mv[U];
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
      Unit xv, gv, mv;
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
      double* pa = partial + (static_cast<long long>(blockIdx.x) * 2 + 0) * g.c + e;
      double* pb = partial + (static_cast<long long>(blockIdx.x) * 2 + 1) * g.c + e;
      if constexpr (PUBLISH) { stat_publish(pa, a); stat_publish(pb, b); }
      else { *pa = a; *pb = b; }
    }
  }
}

template <class F, int V, bool BWD>
__global__ __launch_bounds__(256) void bn_reduce_k(const typename F::elem* __restrict__ x, const typename F::elem* __restrict__ dy, BnGeom g,
                                                   const float* __restrict__ mean, const float* __restrict__ invstd,
                                                   const void* __restrict__ gamma, const void* __restrict__ beta, int pd, int relu,
                                                   double* __restrict__ partial, const typename F::elem* __restrict__ mask_y) {
  __shared__ double red[2][256 * V];
  bn_reduce_rows<F, V, BWD, false>(x, dy, g, mean, invstd, gamma, beta, pd, relu, mask_y, partial, red);
}

// ---- the fold-and-finalise prologues: per-channel constants of the per-element loops, in LDS -------------------------------------------
// (arrays of kBnMaxC floats each, declared by the kernel one by one: as one LDS object they cost the folding kernels two VGPRs;
// y = x * scale + shift would need two of them instead of four and change the rounding)
struct BnFwdLds { float *mean, *is, *gamma, *beta; };
struct BnBwdLds { float *mean, *is, *gamma, *beta, *c1, *c2; };

struct BnRun {   // running statistics in the parameters' format (pd); the apply kernels move these, not BnFwdFin's fp32 pair
  void* running_mean; void* running_var;
};
struct BnBwdOut {   // dgamma / dbeta in the parameters' format (pd); coef: c1 = coef[0][c], c2 = coef[1][c], read where nothing is folded
  void* dgamma; void* dbeta; const float* coef;
  int batch_stats;
};

// conv-epilogue statistics alternate between two slot buffers: the apply launch reads one and clears the other for the next fused
// conv, which runs after it on the stream
template <class F>
__device__ __forceinline__ void bn_clear_slots(double* __restrict__ zero_next, long long zero_count) {
  if constexpr (kIs32<F>) {
    if (zero_next && blockIdx.x == 0)
      for (long long e = threadIdx.x; e < zero_count; e += 256) zero_next[e] = 0.0;
  }
}

// FOLD: batch statistics come from the partials (training), and workgroup 0 stores them and moves the running statistics; otherwise
// mean / invstd are read from memory (eval mode, or statistics that were finalised already: bn_fold.hpp).  COHERENT: as fold_chunk.
template <class F, bool FOLD, bool COHERENT>
__device__ __forceinline__ void bn_fwd_prologue(const BnGeom& g, const double* __restrict__ partial, const BnFwdFin& ff, const BnRun& run,
                                                const void* gamma, const void* beta, int pd, double (*red)[256], const BnFwdLds& sh) {
  const int tid = threadIdx.x, c = g.c;
  const int cfold = c < 256 ? c : 256;
  for (int e0 = 0; e0 < c; e0 += cfold) {
    const int e = e0 + tid;
    float mu_f = 0.f, is_f = 0.f;
    if constexpr (FOLD) {
      double a, b;
      fold_chunk<COHERENT>(g.nblk, c, partial, e0, cfold, red, &a, &b);
      if (tid < cfold && e < c) bn_fwd_channel<F>(a, b, g.n, ff, run.running_mean, run.running_var, pd, e, blockIdx.x == 0, &mu_f, &is_f);
    } else {
      mu_f = (tid < cfold && e < c) ? ff.mean[e] : 0.f;
      is_f = (tid < cfold && e < c) ? ff.invstd[e] : 0.f;
    }
    if (tid < cfold && e < c) {
      sh.mean[e] = mu_f;
      sh.is[e] = is_f;
      sh.gamma[e] = F::par_load(gamma, e, pd, 1.f);
      sh.beta[e] = F::par_load(beta, e, pd, 0.f);
    }
  }
  // momentum=None: every channel above read *num_batches_tracked; the bump must not overtake a channel of another wave
  __syncthreads();
  if (FOLD && blockIdx.x == 0 && tid == 0 && run.running_mean && ff.num_batches_tracked) *ff.num_batches_tracked += 1;
}

// FOLD: (sum dz, sum dz * xhat) come from the partials, and workgroup 0 stores them as dbeta / dgamma; otherwise their means c1, c2 are
// read from out.coef (finalised, with dgamma and dbeta, by the last workgroup of the launch that took the sums).
template <class F, bool FOLD, bool COHERENT>
__device__ __forceinline__ void bn_bwd_prologue(const BnGeom& g, const double* __restrict__ partial, const float* mean, const float* invstd,
                                                const void* gamma, const void* beta, int pd, const BnBwdOut& out, double (*red)[256],
                                                const BnBwdLds& sh) {
  const int tid = threadIdx.x, c = g.c;
  const int cfold = c < 256 ? c : 256;
  for (int e0 = 0; e0 < c; e0 += cfold) {
    const int e = e0 + tid;
    double a = 0.0, b = 0.0;
    if constexpr (FOLD) fold_chunk<COHERENT>(g.nblk, c, partial, e0, cfold, red, &a, &b);
    if (tid < cfold && e < c) {
      if constexpr (FOLD) {
        const double n = static_cast<double>(g.n);
        if (blockIdx.x == 0) {
          F::par_store(out.dbeta, e, pd, a);
          F::par_store(out.dgamma, e, pd, b);
        }
        sh.c1[e] = out.batch_stats ? static_cast<float>(a / n) : 0.f;
        sh.c2[e] = out.batch_stats ? static_cast<float>(b / n) : 0.f;
      } else {
        sh.c1[e] = out.coef[e];
        sh.c2[e] = out.coef[c + e];
      }
      sh.mean[e] = mean[e];
      sh.is[e] = invstd[e];
      sh.gamma[e] = F::par_load(gamma, e, pd, 1.f);
      sh.beta[e] = F::par_load(beta, e, pd, 0.f);
    }
  }
  __syncthreads();
}

// ---- the per-element loops: grid-stride over units of V elements --------------------------------------------------------------------------
// y = relu?((x - mean) * invstd * gamma + beta [+ residual]); the residual form is the tail of a residual block
// (spconv_backbone.py:63-66: out.features += identity; relu) in the same pass.
template <class F, int V>
__device__ __forceinline__ void bn_fwd_rows(const typename F::elem* __restrict__ x, const typename F::elem* __restrict__ residual,
                                            typename F::elem* __restrict__ y, long long units, int c, int relu, const BnFwdLds& sh) {
  using Unit = typename F::template Unit<V>;
  const int cv = c / V;
  for (long long u = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; u < units; u += static_cast<long long>(gridDim.x) * 256) {
    const int col = static_cast<int>(u % cv) * V;
    Unit xv, rv, o;
    xv.load(x + u * V);
    if (residual) rv.load(residual + u * V);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float xhat = (xv.v[i] - sh.mean[col + i]) * sh.is[col + i];
      float t = xhat * sh.gamma[col + i] + sh.beta[col + i];
      if (residual) t = t + rv.v[i];
      o.v[i] = (relu && t <= 0.f) ? 0.f : t;  // NaN passes through, like torch.relu
    }
    o.store(y + u * V);
  }
}

// dx = gamma * invstd * (dz - c1 - xhat * c2), dz = dy * [t > 0] with t the fp32 pre-activation, NOT F::stored(t) (see the file header).
// mask_y / dz_out (the residual form): the ReLU mask comes from the block's output, and dz - the gradient of the identity branch, dy
// or 0: stored exactly - is written beside dx.
template <class F, int V>
__device__ __forceinline__ void bn_bwd_rows(const typename F::elem* __restrict__ x, const typename F::elem* __restrict__ dy,
                                            const typename F::elem* __restrict__ mask_y, typename F::elem* __restrict__ dx,
                                            typename F::elem* __restrict__ dz_out, long long units, int c, int relu, const BnBwdLds& sh) {
  using Unit = typename F::template Unit<V>;
  const int cv = c / V;
  for (long long u = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; u < units; u += static_cast<long long>(gridDim.x) * 256) {
    const int col = static_cast<int>(u % cv) * V;
    Unit xv, gv, mv, o, z;
    xv.load(x + u * V);
    gv.load(dy + u * V);
    if (mask_y) mv.load(mask_y + u * V);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float is = sh.is[col + i], ga = sh.gamma[col + i];
      const float xhat = (xv.v[i] - sh.mean[col + i]) * is;
      const float t = mask_y ? mv.v[i] : xhat * ga + sh.beta[col + i];
      const float dz = (relu && !(t > 0.f)) ? 0.f : gv.v[i];
      z.v[i] = dz;
      o.v[i] = ga * is * (dz - sh.c1[col + i] - xhat * sh.c2[col + i]);
    }
    o.store(dx + u * V);
    if (dz_out) z.store(dz_out + u * V);
  }
}

template <class F, int V, bool FOLD>
__global__ __launch_bounds__(256) void bn_apply_fwd_k(const typename F::elem* __restrict__ x, long long units, BnGeom g,
                                                      const double* __restrict__ partial, BnFwdFin ff, BnRun run, const void* __restrict__ gamma,
                                                      const void* __restrict__ beta, int pd, int relu, typename F::elem* __restrict__ y,
                                                      double* __restrict__ zero_next, long long zero_count,
                                                      const typename F::elem* __restrict__ residual) {
  __shared__ double red[2][256];
  __shared__ float sh_mean[kBnMaxC], sh_is[kBnMaxC], sh_gamma[kBnMaxC], sh_beta[kBnMaxC];
  const BnFwdLds sh{sh_mean, sh_is, sh_gamma, sh_beta};
  bn_clear_slots<F>(zero_next, zero_count);
  bn_fwd_prologue<F, FOLD, false>(g, partial, ff, run, gamma, beta, pd, red, sh);
  bn_fwd_rows<F, V>(x, residual, y, units, g.c, relu, sh);
}

template <class F, int V, bool FOLD>
__global__ __launch_bounds__(256) void bn_apply_bwd_k(const typename F::elem* __restrict__ x, const typename F::elem* __restrict__ dy, long long units,
                                                      BnGeom g, const double* __restrict__ partial, const float* __restrict__ mean,
                                                      const float* __restrict__ invstd, const void* __restrict__ gamma,
                                                      const void* __restrict__ beta, int pd, int relu, BnBwdOut out,
                                                      typename F::elem* __restrict__ dx, double* __restrict__ zero_next, long long zero_count,
                                                      const typename F::elem* __restrict__ mask_y, typename F::elem* __restrict__ dz_out) {
  __shared__ double red[2][256];
  __shared__ float sh_mean[kBnMaxC], sh_is[kBnMaxC], sh_gamma[kBnMaxC], sh_beta[kBnMaxC], sh_c1[kBnMaxC], sh_c2[kBnMaxC];
  const BnBwdLds sh{sh_mean, sh_is, sh_gamma, sh_beta, sh_c1, sh_c2};
  bn_clear_slots<F>(zero_next, zero_count);
  bn_bwd_prologue<F, FOLD, false>(g, partial, mean, invstd, gamma, beta, pd, out, red, sh);
  bn_bwd_rows<F, V>(x, dy, mask_y, dx, dz_out, units, g.c, relu, sh);
}

// One workgroup: the fold + finalisation the last workgroup of a conv launch does (conv_stats_done, sparse_conv.hip), for sums that a
// separate pass took (column counts the conv epilogues do not cover).  Leaves the slots zero like that one.
template <bool BWD>
__global__ __launch_bounds__(256) void bn_finalize_k(double* __restrict__ stats, long long n, int c, BnFwdFin ff, BnBwdFin bf) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x, cfold = c < 256 ? c : 256;
  for (int e0 = 0; e0 < c; e0 += cfold) {
    const int e = e0 + tid;
    double a, b;
    fold_chunk<false>(kStatSlots, c, stats, e0, cfold, red, &a, &b);
    if (tid < cfold && e < c) {
      if (!BWD) {
        float mu, is;
        bn_fwd_channel(a, b, n, ff, e, true, &mu, &is);
      } else {
        const double nn = static_cast<double>(n);
        bf.dbeta[e] = static_cast<float>(a);
        bf.dgamma[e] = static_cast<float>(b);
        bf.coef[e] = bf.batch_stats ? static_cast<float>(a / nn) : 0.f;
        bf.coef[c + e] = bf.batch_stats ? static_cast<float>(b / nn) : 0.f;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < kStatSlots * 2 * c; i += 256) stats[i] = 0.0;
  if (!BWD && tid == 0 && ff.running_mean && ff.num_batches_tracked) *ff.num_batches_tracked += 1;
}

// ---- one launch per BatchNorm pass: reduce, grid barrier, apply ----------------------------------------------------------------------
// The BatchNorms that do not sit behind one of this library's convs (the decoder's Linear -> BatchNorm1d -> ReLU rows, the residual
// tails, every layer whose incoming gradient is a sum of several) took two launches forward and two backward: a reduce pass on <= 64
// workgroups and the apply pass, with the launch gap of two dependent kernels between them (bn_reduce_k<BWD> alone: 25 us x 29 per FV2P
// step).  Here both phases are one kernel of G <= kOneGrid workgroups that are all resident at once (256 threads, 20 KB of LDS: a CU
// holds eight, the chip 2 048 - several such launches from different streams still fit side by side, and kernels that do not wait for
// anybody finish in between).  Phase 1: workgroup b reduces its rows and publishes partial[b] with agent-scope stores (write-through:
// the eight XCD L2s are not coherent with each other), waits for their acknowledgement and counts itself in.  Barrier: one thread per
// workgroup polls the counter with agent-scope loads.  Phase 2: every workgroup folds the G partials (fold_chunk: the same fixed order
// as the two-launch form, so the statistics are bit-identical to it) and applies its share of the rows.  The last workgroup to leave
// resets the two counters.  No fence: nothing but the partials and the counters crosses workgroups.
constexpr int kOneGrid = 128;
// Every workgroup folds ALL partials with loads that bypass its L2: G^2 x 2 c doubles cross the fabric per launch (33 MB at G = 128,
// c = 128: 46 against 33 us for the two-launch forward at 10 000 x 128).  Wide layers therefore run on 32 workgroups (2 MB); what that
// leaves of the chip is enough up to ~2 M elements (tools/bn_time.py), above that the caller keeps reduce + apply.
int one_grid(int c) { return c >= 64 ? 32 : kOneGrid; }

__device__ __forceinline__ void grid_arrive_and_wait(unsigned* counters, unsigned total) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this workgroup's partials have been acknowledged
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(counters, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (__hip_atomic_load(counters, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < total) __builtin_amdgcn_s_sleep(2);
  }
  __syncthreads();
}
__device__ __forceinline__ void grid_leave(unsigned* counters, unsigned total) {
  __syncthreads();
  if (threadIdx.x == 0) {
    if (__hip_atomic_fetch_add(counters + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == total - 1u) {
      __hip_atomic_store(counters, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(counters + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <class F, int V>
__global__ __launch_bounds__(256) void bn_one_fwd_k(const typename F::elem* __restrict__ x, long long units, BnGeom g, double* __restrict__ partial,
                                                    unsigned* __restrict__ counters, BnFwdFin ff, BnRun run, const void* __restrict__ gamma,
                                                    const void* __restrict__ beta, int pd, int relu, typename F::elem* __restrict__ y,
                                                    const typename F::elem* __restrict__ residual) {
  __shared__ double red1[2][256 * V];
  __shared__ float sh_mean[kBnMaxC], sh_is[kBnMaxC], sh_gamma[kBnMaxC], sh_beta[kBnMaxC];
  const BnFwdLds sh{sh_mean, sh_is, sh_gamma, sh_beta};
  bn_reduce_rows<F, V, false, true>(x, nullptr, g, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, partial, red1);
  grid_arrive_and_wait(counters, gridDim.x);
  bn_fwd_prologue<F, true, true>(g, partial, ff, run, gamma, beta, pd, reinterpret_cast<double (*)[256]>(&red1[0][0]), sh);
  bn_fwd_rows<F, V>(x, residual, y, units, g.c, relu, sh);
  grid_leave(counters, gridDim.x);
}

template <class F, int V>
__global__ __launch_bounds__(256) void bn_one_bwd_k(const typename F::elem* __restrict__ x, const typename F::elem* __restrict__ dy, long long units,
                                                    BnGeom g, double* __restrict__ partial, unsigned* __restrict__ counters,
                                                    const float* __restrict__ mean, const float* __restrict__ invstd, const void* __restrict__ gamma,
                                                    const void* __restrict__ beta, int pd, int relu, BnBwdOut out, typename F::elem* __restrict__ dx,
                                                    const typename F::elem* __restrict__ mask_y, typename F::elem* __restrict__ dz_out) {
  __shared__ double red1[2][256 * V];
  __shared__ float sh_mean[kBnMaxC], sh_is[kBnMaxC], sh_gamma[kBnMaxC], sh_beta[kBnMaxC], sh_c1[kBnMaxC], sh_c2[kBnMaxC];
  const BnBwdLds sh{sh_mean, sh_is, sh_gamma, sh_beta, sh_c1, sh_c2};
  bn_reduce_rows<F, V, true, true>(x, dy, g, mean, invstd, gamma, beta, pd, relu, mask_y, partial, red1);
  grid_arrive_and_wait(counters, gridDim.x);
  bn_bwd_prologue<F, true, true>(g, partial, mean, invstd, gamma, beta, pd, out, reinterpret_cast<double (*)[256]>(&red1[0][0]), sh);
  bn_bwd_rows<F, V>(x, dy, mask_y, dx, dz_out, units, g.c, relu, sh);
  grid_leave(counters, gridDim.x);
}

// ---- two launches, the first one wide: reduce on up to 512 workgroups with the sums finalised by its last workgroups, then apply -------
// The decoder's Linear -> BatchNorm1d -> ReLU rows are 49 152 x 64 / 128 (12 - 25 MB): too large for the one-launch form, and their
// reduce pass ran on <= 64 workgroups because EVERY apply workgroup folded all the partials (36.5 us backward, 18.5 us forward:
// ~1.4 TB/s).  With the finalisation of bn_fold.hpp the partials are folded once, by the reduce launch's own last workgroups, so the
// reduce can be as wide as the tensor wants and the apply pass reads finished numbers (mean / invstd, or c1 / c2).
constexpr int kWideGrid = 512;
template <class F, int V, bool BWD>
__global__ __launch_bounds__(256) void bn_reduce_fin_k(const typename F::elem* __restrict__ x, const typename F::elem* __restrict__ dy, BnGeom g,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd,
                                                       const void* __restrict__ gamma, const void* __restrict__ beta, int pd, int relu,
                                                       const typename F::elem* __restrict__ mask_y, double* __restrict__ rows,
                                                       double* __restrict__ gslots, unsigned* __restrict__ counter, int groups, FinOut fo) {
  __shared__ double red1[2][256 * V];
  __shared__ unsigned flag;
  bn_reduce_rows<F, V, BWD, true>(x, dy, g, mean, invstd, gamma, beta, pd, relu, mask_y, rows, red1);   // publishes row blockIdx.x of rows [nblk][2][c]
  __syncthreads();
  for (int e0 = 0; e0 < g.c; e0 += 128) {   // the protocol handles <= 128 columns a pass; every pass sees all workgroups (counters reset in between)
    FinOut f = fo;
    const int cc = min(128, g.c - e0);
    f.ff.mean = fo.ff.mean ? fo.ff.mean + e0 : nullptr; f.ff.invstd = fo.ff.invstd ? fo.ff.invstd + e0 : nullptr;
    f.ff.running_mean = fo.ff.running_mean ? fo.ff.running_mean + e0 : nullptr; f.ff.running_var = fo.ff.running_var ? fo.ff.running_var + e0 : nullptr;
    f.bf.dgamma = fo.bf.dgamma ? fo.bf.dgamma + e0 : nullptr; f.bf.dbeta = fo.bf.dbeta ? fo.bf.dbeta + e0 : nullptr; f.bf.coef = fo.bf.coef ? fo.bf.coef + e0 : nullptr;
    f.bump = fo.bump && (e0 + 128 >= g.c);
    fin_rows_done(rows + e0, gslots + e0, counter + (e0 / 128) * ((1 + kFinSubs) * kFinStride), static_cast<int>(blockIdx.x), static_cast<int>(gridDim.x), 1, groups,
                  cc, g.c, &flag, reinterpret_cast<double (*)[256]>(&red1[0][0]), f);
    __syncthreads();
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
// the reduce geometry at v elements per lane; -1: more channels than the width allows
int bn_geom(int64_t n, int c, int v, BnGeom* g, int max_blocks) {
  g->n = n; g->c = c;
  g->tcols = static_cast<int>(ceil_div(c, v));
  if (g->tcols > 256 || c > kBnMaxC) return -1;
  g->rpp = 256 / g->tcols;
  // >= 8 rows per row lane per workgroup, at most max_blocks workgroups (kBnPartials where every apply workgroup re-folds the partials)
  int64_t nblk = ceil_div(n, static_cast<int64_t>(g->rpp) * 8);
  if (nblk > max_blocks) nblk = max_blocks;
  if (nblk < 1) nblk = 1;
  g->rows_per_block = ceil_div(n, nblk);
  g->nblk = static_cast<int>(ceil_div(n, g->rows_per_block));
  return 0;
}

unsigned apply_blocks(long long units) {
  // grid-stride, ~4 units per thread, at most 2 workgroups per CU worth of fold prologues
  const int64_t b = ceil_div(units, 256 * 4);
  return static_cast<unsigned>(b > 512 ? 512 : (b < 1 ? 1 : b));
}

using Ptrs = std::initializer_list<const void*>;

// What an entry point works out before it launches: the width (the format's 16-byte vector when c is a multiple of it and every
// tensor of the call - a null one is not there - is 16-byte aligned, one element otherwise), the reduce geometry on at most max_blocks
// workgroups, and the apply pass's units and grid.
struct BnPlan {
  BnGeom g; bool vec; long long units; unsigned blocks;
};
int bn_plan(const char* who, int dtype, int64_t n, int c, Ptrs tensors, int max_blocks, BnPlan* p) {
  const int kvec = dtype == 0 ? F32::kVec : Fmt16<H16>::kVec;
  p->vec = c % kvec == 0;
  for (const void* t : tensors) p->vec = p->vec && aligned16(t);
  const int v = p->vec ? kvec : 1;
  FV2P_REQUIRE(bn_geom(n, c, v, &p->g, max_blocks) == 0, FV2P_ELIMIT, "%s: c=%d exceeds %d", who, c, p->vec ? kBnMaxC : 256);
  p->units = n * c / v;
  p->blocks = apply_blocks(p->units);
  return 0;
}

// fn(format, width) for the call's format (dtype 0: fp32) at the plan's width
template <class F, class Fn>
void bn_width(bool vec, Fn fn) {
  if (vec) fn(F{}, std::integral_constant<int, F::kVec>{});
  else fn(F{}, std::integral_constant<int, 1>{});
}
template <class Fn>
void bn_dispatch(int dtype, bool vec, Fn fn) {
  if (dtype == 0) bn_width<F32>(vec, fn);
  else if (dtype == FV2P_DT_F16) bn_width<Fmt16<H16>>(vec, fn);
  else bn_width<Fmt16<B16>>(vec, fn);
}

// the argument checks the entry points share
#define BN_TRY(expr) do { if (const int rc__ = (expr)) return rc__; } while (0)
int bn_check_nc(const char* who, int64_t n, int c, int64_t n_min) {
  FV2P_REQUIRE(n >= n_min && c >= 1, FV2P_EINVAL, "%s: n=%lld c=%d", who, static_cast<long long>(n), c);
  return 0;
}
int bn_check_ptrs(const char* who, Ptrs required) {
  for (const void* p : required) FV2P_REQUIRE(p, FV2P_EINVAL, "%s: null pointer", who);
  return 0;
}
int bn_check_running(const char* who, const void* running_mean, const void* running_var) {
  FV2P_REQUIRE((running_mean == nullptr) == (running_var == nullptr), FV2P_EINVAL, "%s: running_mean and running_var come together", who);
  return 0;
}
int bn_check_ws(const char* who, size_t ws_bytes, size_t need) {
  FV2P_REQUIRE(ws_bytes >= need, FV2P_EWORKSPACE, "%s: workspace %lld < %lld", who, static_cast<long long>(ws_bytes), static_cast<long long>(need));
  return 0;
}
int bn_check_formats(const char* who, int dtype, int param_dtype) {   // the `_h` entry points
  FV2P_DT16_OK(who, dtype);
  FV2P_REQUIRE(param_dtype == 0 || param_dtype == dtype, FV2P_EINVAL, "%s: param_dtype %d is neither 0 (fp32) nor the call's dtype %d", who,
               param_dtype, dtype);
  return 0;
}

size_t bn_ws_bytes(int slots, int c, int coef_floats = 0) {
  Sizer s;
  s.take<double>(static_cast<size_t>(slots) * 2 * (c > 0 ? c : 1));
  if (coef_floats) s.take<float>(static_cast<size_t>(coef_floats) * (c > 0 ? c : 1));
  return s.bytes();
}

template <class F>
const typename F::elem* rd(const void* p) { return static_cast<const typename F::elem*>(p); }
template <class F>
typename F::elem* wr(void* p) { return static_cast<typename F::elem*>(p); }

struct BnFwdArgs {   // the tensors and options of a forward pass (a null residual / zero_next is not there)
  const void* x; const void* gamma; const void* beta; int pd, relu; const void* residual; void* y;
  double* zero_next = nullptr; long long zero_count = 0;
};
struct BnBwdArgs {
  const void* x; const void* dy; const float* mean; const float* invstd; const void* gamma; const void* beta; int pd, relu;
  const void* mask_y; void* dx; void* dz_out;
  double* zero_next = nullptr; long long zero_count = 0;
};

template <class F, int V, bool BWD>
void launch_reduce(const BnGeom& g, const BnBwdArgs& a, double* partial, hipStream_t stream) {   // forward: x alone is looked at
  hipLaunchKernelGGL((bn_reduce_k<F, V, BWD>), dim3(g.nblk), dim3(256), 0, stream, rd<F>(a.x), rd<F>(a.dy), g, a.mean, a.invstd, a.gamma, a.beta, a.pd,
                     a.relu, partial, rd<F>(a.mask_y));
}
template <class F, int V, bool FOLD>
void launch_apply_fwd(const BnPlan& p, const BnFwdArgs& a, const double* partial, const BnFwdFin& ff, const BnRun& run, hipStream_t stream) {
  hipLaunchKernelGGL((bn_apply_fwd_k<F, V, FOLD>), dim3(p.blocks), dim3(256), 0, stream, rd<F>(a.x), p.units, p.g, partial, ff, run, a.gamma, a.beta, a.pd,
                     a.relu, wr<F>(a.y), a.zero_next, a.zero_count, rd<F>(a.residual));
}
template <class F, int V, bool FOLD>
void launch_apply_bwd(const BnPlan& p, const BnBwdArgs& a, const double* partial, const BnBwdOut& o, hipStream_t stream) {
  hipLaunchKernelGGL((bn_apply_bwd_k<F, V, FOLD>), dim3(p.blocks), dim3(256), 0, stream, rd<F>(a.x), rd<F>(a.dy), p.units, p.g, partial, a.mean, a.invstd,
                     a.gamma, a.beta, a.pd, a.relu, o, wr<F>(a.dx), a.zero_next, a.zero_count, rd<F>(a.mask_y), wr<F>(a.dz_out));
}
const BnBwdArgs fwd_rows(const void* x) { return BnBwdArgs{x, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr}; }

// ---- the two-launch form, every format: bodies of fv2p_batchnorm_forward / _forward_h, _apply / _apply_res / _apply_h and
// _backward / _backward_res / _backward_h.  n_min: 1 where an empty tensor is an error, 0 where it is a call that does nothing.
int bn_forward(const char* who, int dtype, int param_dtype, int64_t n_min, const void* x, int64_t n, int c, float eps, float momentum,
               const void* gamma, const void* beta, int relu, const void* residual, void* running_mean, void* running_var,
               int64_t* num_batches_tracked, float* mean, float* invstd, void* y, void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  BN_TRY(bn_check_nc(who, n, c, n_min));
  if (n == 0) return 0;
  BN_TRY(bn_check_ptrs(who, {x, y, mean, invstd, ws}));
  BN_TRY(bn_check_running(who, running_mean, running_var));
  BN_TRY(bn_check_ws(who, ws_bytes, bn_ws_bytes(kBnPartials, c)));
  BnPlan p;
  BN_TRY(bn_plan(who, dtype, n, c, {x, y, residual}, kBnPartials, &p));
  double* partial = Carver(ws, ws_bytes).take<double>(static_cast<size_t>(kBnPartials) * 2 * c);
  const BnFwdFin ff{mean, invstd, nullptr, nullptr, reinterpret_cast<long long*>(num_batches_tracked), momentum, eps};
  const BnRun run{running_mean, running_var};
  const BnFwdArgs a{x, gamma, beta, param_dtype != 0, relu, residual, y};
  bn_dispatch(dtype, p.vec, [&](auto f, auto v) {
    using F = decltype(f);
    launch_reduce<F, decltype(v)::value, false>(p.g, fwd_rows(x), partial, stream);
    launch_apply_fwd<F, decltype(v)::value, true>(p, a, partial, ff, run, stream);
  });
  FV2P_LAUNCH_CHECK();
  return 0;
}

// y = relu?((x - mean) * invstd * gamma + beta [+ residual]) with given mean / invstd: eval mode, or batch statistics the producing
// conv's last workgroup finalised (fv2p_sparse_conv_rows_bnfin).  One launch, no fold.
int bn_apply(const char* who, int dtype, int param_dtype, const void* x, int64_t n, int c, const float* mean, const float* invstd, const void* gamma,
             const void* beta, int relu, const void* residual, void* y, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  BN_TRY(bn_check_nc(who, n, c, 0));
  if (n == 0) return 0;
  BN_TRY(bn_check_ptrs(who, {x, y, mean, invstd}));
  BnPlan p;
  BN_TRY(bn_plan(who, dtype, n, c, {x, y, residual}, kBnPartials, &p));
  const BnFwdFin ff{const_cast<float*>(mean), const_cast<float*>(invstd), nullptr, nullptr, nullptr, 0.f, 0.f};
  const BnFwdArgs a{x, gamma, beta, param_dtype != 0, relu, residual, y};
  bn_dispatch(dtype, p.vec, [&](auto f, auto v) { launch_apply_fwd<decltype(f), decltype(v)::value, false>(p, a, nullptr, ff, BnRun{nullptr, nullptr}, stream); });
  FV2P_LAUNCH_CHECK();
  return 0;
}

// mask_y (NULL = recompute the ReLU mask from x) and dz_out (NULL = not wanted): the residual form, out = relu(bn(x) + identity) - dz =
// dout * [out > 0] is the identity branch's gradient and the BatchNorm's incoming one.  Two launches (reduce, apply).
int bn_backward(const char* who, int dtype, int param_dtype, int64_t n_min, const void* x, const void* dy, int64_t n, int c, const float* mean,
                const float* invstd, const void* gamma, const void* beta, int relu, int batch_stats, const void* mask_y, void* dx, void* dz_out,
                void* dgamma, void* dbeta, void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  BN_TRY(bn_check_nc(who, n, c, n_min));
  if (n == 0) return 0;
  BN_TRY(bn_check_ptrs(who, {x, dy, mean, invstd, dx, dgamma, dbeta, ws}));
  BN_TRY(bn_check_ws(who, ws_bytes, bn_ws_bytes(kBnPartials, c)));
  BnPlan p;
  BN_TRY(bn_plan(who, dtype, n, c, {x, dy, dx, mask_y, dz_out}, kBnPartials, &p));
  double* partial = Carver(ws, ws_bytes).take<double>(static_cast<size_t>(kBnPartials) * 2 * c);
  const BnBwdArgs a{x, dy, mean, invstd, gamma, beta, param_dtype != 0, relu, mask_y, dx, dz_out};
  const BnBwdOut o{dgamma, dbeta, nullptr, batch_stats};
  bn_dispatch(dtype, p.vec, [&](auto f, auto v) {
    using F = decltype(f);
    launch_reduce<F, decltype(v)::value, true>(p.g, a, partial, stream);
    launch_apply_bwd<F, decltype(v)::value, true>(p, a, partial, o, stream);
  });
  FV2P_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace fv2p

using namespace fv2p;

extern "C" size_t fv2p_batchnorm_ws_bytes(int64_t n, int c) { (void)n; return bn_ws_bytes(kBnPartials, c); }
extern "C" size_t fv2p_batchnorm_h_ws_bytes(int64_t n, int c) { (void)n; return bn_ws_bytes(kBnPartials, c); }
extern "C" size_t fv2p_batchnorm_one_ws_bytes(int c) { return bn_ws_bytes(kOneGrid, c); }
extern "C" size_t fv2p_batchnorm_wide_ws_bytes(int c) { return bn_ws_bytes(kWideGrid + kFinSubs, c, 2); }   // + c1, c2 of the backward pass
extern "C" int fv2p_batchnorm_wide_counter_words(int c) { return static_cast<int>(((c > 0 ? c : 1) + 127) / 128 * (1 + kFinSubs) * kFinStride); }

extern "C" int fv2p_batchnorm_forward(const float* x, int64_t n, int c, float eps, float momentum, const float* gamma, const float* beta,
                                      int relu, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean,
                                      float* invstd, float* y, void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  return bn_forward("batchnorm_forward", 0, 0, 1, x, n, c, eps, momentum, gamma, beta, relu, nullptr, running_mean, running_var, num_batches_tracked, mean,
                    invstd, y, ws, ws_bytes, stream);
}
extern "C" int fv2p_batchnorm_forward_h(const void* x, int64_t n, int c, float eps, float momentum, const void* gamma, const void* beta, int relu,
                                        const void* residual, void* running_mean, void* running_var, int64_t* num_batches_tracked, float* mean,
                                        float* invstd, void* y, int dtype, int param_dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  BN_TRY(bn_check_formats("batchnorm_forward_h", dtype, param_dtype));
  return bn_forward("batchnorm_forward_h", dtype, param_dtype, 0, x, n, c, eps, momentum, gamma, beta, relu, residual, running_mean, running_var,
                    num_batches_tracked, mean, invstd, y, ws, ws_bytes, stream);
}

extern "C" int fv2p_batchnorm_apply(const float* x, int64_t n, int c, const float* mean, const float* invstd, const float* gamma,
                                    const float* beta, int relu, float* y, fv2p_stream_t stream) {
  return bn_apply("batchnorm_apply", 0, 0, x, n, c, mean, invstd, gamma, beta, relu, nullptr, y, stream);
}
extern "C" int fv2p_batchnorm_apply_res(const float* x, int64_t n, int c, const float* mean, const float* invstd, const float* gamma,
                                        const float* beta, int relu, const float* residual, float* y, fv2p_stream_t stream) {
  return bn_apply("batchnorm_apply_res", 0, 0, x, n, c, mean, invstd, gamma, beta, relu, residual, y, stream);
}
extern "C" int fv2p_batchnorm_apply_h(const void* x, int64_t n, int c, const float* mean, const float* invstd, const void* gamma, const void* beta,
                                      int relu, const void* residual, void* y, int dtype, int param_dtype, fv2p_stream_t stream) {
  BN_TRY(bn_check_formats("batchnorm_apply_h", dtype, param_dtype));
  return bn_apply("batchnorm_apply_h", dtype, param_dtype, x, n, c, mean, invstd, gamma, beta, relu, residual, y, stream);
}

extern "C" int fv2p_batchnorm_backward(const float* x, const float* dy, int64_t n, int c, const float* mean, const float* invstd,
                                       const float* gamma, const float* beta, int relu, int batch_stats, float* dx, float* dgamma,
                                       float* dbeta, void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  return bn_backward("batchnorm_backward", 0, 0, 1, x, dy, n, c, mean, invstd, gamma, beta, relu, batch_stats, nullptr, dx, nullptr, dgamma, dbeta, ws,
                     ws_bytes, stream);
}
// Backward of out = relu(bn(x) + identity) (the tail of a residual block): two launches instead of torch's threshold_backward + the two
// of fv2p_batchnorm_backward.
extern "C" int fv2p_batchnorm_backward_res(const float* x, const float* out, const float* dout, int64_t n, int c, const float* mean,
                                           const float* invstd, const float* gamma, const float* beta, int batch_stats, float* dx, float* dz,
                                           float* dgamma, float* dbeta, void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  BN_TRY(bn_check_ptrs("batchnorm_backward_res", {out, dz}));
  return bn_backward("batchnorm_backward_res", 0, 0, 1, x, dout, n, c, mean, invstd, gamma, beta, 1, batch_stats, out, dx, dz, dgamma, dbeta, ws, ws_bytes,
                     stream);
}
extern "C" int fv2p_batchnorm_backward_h(const void* x, const void* dy, int64_t n, int c, const float* mean, const float* invstd, const void* gamma,
                                         const void* beta, int relu, int batch_stats, const void* mask_y, void* dx, void* dz_out, void* dgamma,
                                         void* dbeta, int dtype, int param_dtype, void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  BN_TRY(bn_check_formats("batchnorm_backward_h", dtype, param_dtype));
  return bn_backward("batchnorm_backward_h", dtype, param_dtype, 0, x, dy, n, c, mean, invstd, gamma, beta, relu, batch_stats, mask_y, dx, dz_out, dgamma,
                     dbeta, ws, ws_bytes, stream);
}

// ---- fp32 rows behind a conv of this library: the sums come from its epilogue, or are finalised by it -------------------------------------
// column sums of x into the slot layout of the conv-epilogue statistics (slots beyond the reduce grid stay as they are: zero)
int fv2p::bn_column_sums(const float* x, int64_t n, int c, double* stats, hipStream_t stream) {
  BnPlan p;
  BN_TRY(bn_plan("batchnorm", 0, n, c, {x}, kStatSlots, &p));
  bn_width<F32>(p.vec, [&](auto f, auto v) { launch_reduce<decltype(f), decltype(v)::value, false>(p.g, fwd_rows(x), stats, stream); });
  FV2P_LAUNCH_CHECK();
  return 0;
}

// (sum dz, sum dz * xhat) into the same slot layout, for a backward-data conv that could not take them in its epilogue
int fv2p::bn_backward_sums(const float* x, const float* dy, int64_t n, int c, const float* mean, const float* invstd, const float* gamma,
                           const float* beta, int relu, double* stats, hipStream_t stream) {
  BnPlan p;
  BN_TRY(bn_plan("batchnorm", 0, n, c, {x, dy}, kStatSlots, &p));
  const BnBwdArgs a{x, dy, mean, invstd, gamma, beta, 0, relu, nullptr, nullptr, nullptr};
  bn_width<F32>(p.vec, [&](auto f, auto v) { launch_reduce<decltype(f), decltype(v)::value, true>(p.g, a, stats, stream); });
  FV2P_LAUNCH_CHECK();
  return 0;
}

int fv2p::bn_finalize_forward(double* stats, int64_t n, int c, const BnFwdFin& ff, hipStream_t stream) {
  FV2P_REQUIRE(c <= kBnMaxC, FV2P_ELIMIT, "batchnorm: c=%d exceeds %d", c, kBnMaxC);
  hipLaunchKernelGGL((bn_finalize_k<false>), dim3(1), dim3(256), 0, stream, stats, static_cast<long long>(n), c, ff, BnBwdFin{nullptr, nullptr, nullptr, 1});
  FV2P_LAUNCH_CHECK();
  return 0;
}
int fv2p::bn_finalize_backward(double* stats, int64_t n, int c, const BnBwdFin& bf, hipStream_t stream) {
  FV2P_REQUIRE(c <= kBnMaxC, FV2P_ELIMIT, "batchnorm: c=%d exceeds %d", c, kBnMaxC);
  hipLaunchKernelGGL((bn_finalize_k<true>), dim3(1), dim3(256), 0, stream, stats, static_cast<long long>(n), c, BnFwdFin{nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f}, bf);
  FV2P_LAUNCH_CHECK();
  return 0;
}

// the apply launch alone: every one of the kStatSlots slots is folded (untouched ones hold zeros), the other slot buffer cleared
extern "C" int fv2p_batchnorm_forward_stats(const float* x, int64_t n, int c, float eps, float momentum, const float* gamma, const float* beta,
                                            int relu, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean,
                                            float* invstd, float* y, const double* stats, double* zero_next, int64_t zero_count,
                                            fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const char* who = "batchnorm_forward_stats";
  BN_TRY(bn_check_nc(who, n, c, 1));
  BN_TRY(bn_check_ptrs(who, {x, y, mean, invstd, stats}));
  BN_TRY(bn_check_running(who, running_mean, running_var));
  BnPlan p;
  BN_TRY(bn_plan(who, 0, n, c, {x, y}, kBnPartials, &p));
  p.g.nblk = kStatSlots;
  const BnFwdFin ff{mean, invstd, nullptr, nullptr, reinterpret_cast<long long*>(num_batches_tracked), momentum, eps};
  const BnFwdArgs a{x, gamma, beta, 0, relu, nullptr, y, zero_next, static_cast<long long>(zero_count)};
  bn_width<F32>(p.vec, [&](auto f, auto v) { launch_apply_fwd<decltype(f), decltype(v)::value, true>(p, a, stats, ff, BnRun{running_mean, running_var}, stream); });
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" int fv2p_batchnorm_backward_stats(const float* x, const float* dy, int64_t n, int c, const float* mean, const float* invstd,
                                             const float* gamma, const float* beta, int relu, int batch_stats, float* dx, float* dgamma,
                                             float* dbeta, const double* stats, double* zero_next, int64_t zero_count, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const char* who = "batchnorm_backward_stats";
  BN_TRY(bn_check_nc(who, n, c, 1));
  BN_TRY(bn_check_ptrs(who, {x, dy, mean, invstd, dx, dgamma, dbeta, stats}));
  BnPlan p;
  BN_TRY(bn_plan(who, 0, n, c, {x, dy, dx}, kBnPartials, &p));
  p.g.nblk = kStatSlots;
  const BnBwdArgs a{x, dy, mean, invstd, gamma, beta, 0, relu, nullptr, dx, nullptr, zero_next, static_cast<long long>(zero_count)};
  const BnBwdOut o{dgamma, dbeta, nullptr, batch_stats};
  bn_width<F32>(p.vec, [&](auto f, auto v) { launch_apply_bwd<decltype(f), decltype(v)::value, true>(p, a, stats, o, stream); });
  FV2P_LAUNCH_CHECK();
  return 0;
}

// dx = gamma * invstd * (dz - c1 - xhat * c2) with c1 = coef[0][c], c2 = coef[1][c] finalised (with dgamma / dbeta) by the last
// workgroup of the backward-data conv that took the sums (fv2p_sparse_conv_rows_bnbwd_fin).  One launch, no fold.
extern "C" int fv2p_batchnorm_backward_fin(const float* x, const float* dy, int64_t n, int c, const float* mean, const float* invstd,
                                           const float* gamma, const float* beta, int relu, const float* coef, float* dx,
                                           fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const char* who = "batchnorm_backward_fin";
  BN_TRY(bn_check_nc(who, n, c, 1));
  BN_TRY(bn_check_ptrs(who, {x, dy, mean, invstd, dx, coef}));
  BnPlan p;
  BN_TRY(bn_plan(who, 0, n, c, {x, dy, dx}, kBnPartials, &p));
  const BnBwdArgs a{x, dy, mean, invstd, gamma, beta, 0, relu, nullptr, dx, nullptr};
  const BnBwdOut o{nullptr, nullptr, coef, 1};
  bn_width<F32>(p.vec, [&](auto f, auto v) { launch_apply_bwd<decltype(f), decltype(v)::value, false>(p, a, nullptr, o, stream); });
  FV2P_LAUNCH_CHECK();
  return 0;
}

// ---- fp32 rows, one launch (bn_one_*) or the wide reduce (bn_reduce_fin_k) ------------------------------------------------------------------
extern "C" int fv2p_batchnorm_one_pays(int64_t n, int c, int backward) {
  // measured against the wide reduce + apply (tools/bn_time.py, profiles/r06_bn_time.txt): backward 64 against 73 us at 35 000 x 16 and
  // 59 against 70 at 39 000 x 32, but 81 against 72 at 22 000 x 64 and 82 against 69 at 10 000 x 128 (32 workgroups are too few for
  // the two passes over the tensor); forward equal at 16 columns, behind from 32 on
  const int64_t elems = n * c;
  if (elems > (2ll << 20)) return 0;
  return backward ? (c <= 32 ? 1 : 0) : (c <= 16 ? 1 : 0);
}

// fv2p_batchnorm_forward (+ optional residual) in ONE launch.  counters: two zeroed device words the caller keeps per stream (zero again
// when the launch ends).  Same statistics, bit for bit, as the two-launch form on the same number of partials.
extern "C" int fv2p_batchnorm_forward_one(const float* x, int64_t n, int c, float eps, float momentum, const float* gamma, const float* beta,
                                          int relu, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean,
                                          float* invstd, const float* residual, float* y, void* ws, size_t ws_bytes, unsigned* counters,
                                          fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const char* who = "batchnorm_forward_one";
  BN_TRY(bn_check_nc(who, n, c, 1));
  BN_TRY(bn_check_ptrs(who, {x, y, mean, invstd, ws, counters}));
  BN_TRY(bn_check_running(who, running_mean, running_var));
  BN_TRY(bn_check_ws(who, ws_bytes, fv2p_batchnorm_one_ws_bytes(c)));
  BnPlan p;
  BN_TRY(bn_plan(who, 0, n, c, {x, y, residual}, one_grid(c), &p));
  double* partial = Carver(ws, ws_bytes).take<double>(static_cast<size_t>(kOneGrid) * 2 * c);
  const BnFwdFin ff{mean, invstd, nullptr, nullptr, reinterpret_cast<long long*>(num_batches_tracked), momentum, eps};
  bn_width<F32>(p.vec, [&](auto f, auto v) {
    hipLaunchKernelGGL((bn_one_fwd_k<decltype(f), decltype(v)::value>), dim3(p.g.nblk), dim3(256), 0, stream, x, p.units, p.g, partial, counters, ff,
                       BnRun{running_mean, running_var}, gamma, beta, 0, relu, y, residual);
  });
  FV2P_LAUNCH_CHECK();
  return 0;
}

// fv2p_batchnorm_backward / _backward_res in ONE launch: mask_y and dz_out as in bn_backward.
extern "C" int fv2p_batchnorm_backward_one(const float* x, const float* dy, int64_t n, int c, const float* mean, const float* invstd,
                                           const float* gamma, const float* beta, int relu, int batch_stats, const float* mask_y, float* dx,
                                           float* dz_out, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, unsigned* counters,
                                           fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const char* who = "batchnorm_backward_one";
  BN_TRY(bn_check_nc(who, n, c, 1));
  BN_TRY(bn_check_ptrs(who, {x, dy, mean, invstd, dx, dgamma, dbeta, ws, counters}));
  BN_TRY(bn_check_ws(who, ws_bytes, fv2p_batchnorm_one_ws_bytes(c)));
  BnPlan p;
  BN_TRY(bn_plan(who, 0, n, c, {x, dy, dx, mask_y, dz_out}, one_grid(c), &p));
  double* partial = Carver(ws, ws_bytes).take<double>(static_cast<size_t>(kOneGrid) * 2 * c);
  const BnBwdOut o{dgamma, dbeta, nullptr, batch_stats};
  bn_width<F32>(p.vec, [&](auto f, auto v) {
    hipLaunchKernelGGL((bn_one_bwd_k<decltype(f), decltype(v)::value>), dim3(p.g.nblk), dim3(256), 0, stream, x, dy, p.units, p.g, partial, counters, mean,
                       invstd, gamma, beta, 0, relu, o, dx, mask_y, dz_out);
  });
  FV2P_LAUNCH_CHECK();
  return 0;
}

// fv2p_batchnorm_forward (+ optional residual) with the wide reduce: two launches, nothing folded in the apply pass.  counters:
// fv2p_batchnorm_wide_counter_words(c) zeroed device words the caller keeps per stream (zero again when the reduce launch ends).
extern "C" int fv2p_batchnorm_forward_wide(const float* x, int64_t n, int c, float eps, float momentum, const float* gamma, const float* beta,
                                           int relu, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean,
                                           float* invstd, const float* residual, float* y, void* ws, size_t ws_bytes, unsigned* counters,
                                           fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const char* who = "batchnorm_forward_wide";
  BN_TRY(bn_check_nc(who, n, c, 1));
  BN_TRY(bn_check_ptrs(who, {x, y, mean, invstd, ws, counters}));
  BN_TRY(bn_check_running(who, running_mean, running_var));
  BN_TRY(bn_check_ws(who, ws_bytes, fv2p_batchnorm_wide_ws_bytes(c)));
  BnPlan p;
  BN_TRY(bn_plan(who, 0, n, c, {x, y, residual}, kWideGrid, &p));
  double* rows = Carver(ws, ws_bytes).take<double>(static_cast<size_t>(kWideGrid + kFinSubs) * 2 * c);
  double* gslots = rows + static_cast<size_t>(kWideGrid) * 2 * c;
  FinOut fo;
  fo.bwd = 0; fo.n = n; fo.bump = 1; fo.coef_ld = c;
  fo.ff = BnFwdFin{mean, invstd, running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked), momentum, eps};
  fo.bf = BnBwdFin{nullptr, nullptr, nullptr, 1};
  const int groups = p.g.nblk > 256 ? 32 : 16;
  const BnFwdFin ffa{mean, invstd, nullptr, nullptr, nullptr, 0.f, 0.f};
  const BnFwdArgs a{x, gamma, beta, 0, relu, residual, y};
  bn_width<F32>(p.vec, [&](auto f, auto v) {
    hipLaunchKernelGGL((bn_reduce_fin_k<decltype(f), decltype(v)::value, false>), dim3(p.g.nblk), dim3(256), 0, stream, x, nullptr, p.g, nullptr, nullptr,
                       nullptr, nullptr, 0, 0, nullptr, rows, gslots, counters, groups, fo);
    launch_apply_fwd<decltype(f), decltype(v)::value, false>(p, a, nullptr, ffa, BnRun{nullptr, nullptr}, stream);
  });
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" int fv2p_batchnorm_backward_wide(const float* x, const float* dy, int64_t n, int c, const float* mean, const float* invstd,
                                            const float* gamma, const float* beta, int relu, int batch_stats, const float* mask_y, float* dx,
                                            float* dz_out, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, unsigned* counters,
                                            fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const char* who = "batchnorm_backward_wide";
  BN_TRY(bn_check_nc(who, n, c, 1));
  BN_TRY(bn_check_ptrs(who, {x, dy, mean, invstd, dx, dgamma, dbeta, ws, counters}));
  BN_TRY(bn_check_ws(who, ws_bytes, fv2p_batchnorm_wide_ws_bytes(c)));
  BnPlan p;
  BN_TRY(bn_plan(who, 0, n, c, {x, dy, dx, mask_y, dz_out}, kWideGrid, &p));
  Carver cv(ws, ws_bytes);
  double* rows = cv.take<double>(static_cast<size_t>(kWideGrid + kFinSubs) * 2 * c);
  double* gslots = rows + static_cast<size_t>(kWideGrid) * 2 * c;
  float* coef = cv.take<float>(2 * static_cast<size_t>(c));
  FinOut fo;
  fo.bwd = 1; fo.n = n; fo.bump = 0; fo.coef_ld = c;
  fo.ff = BnFwdFin{nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f};
  fo.bf = BnBwdFin{dgamma, dbeta, coef, batch_stats};
  const int groups = p.g.nblk > 256 ? 32 : 16;
  const BnBwdArgs a{x, dy, mean, invstd, gamma, beta, 0, relu, mask_y, dx, dz_out};
  const BnBwdOut o{nullptr, nullptr, coef, batch_stats};
  bn_width<F32>(p.vec, [&](auto f, auto v) {
    hipLaunchKernelGGL((bn_reduce_fin_k<decltype(f), decltype(v)::value, true>), dim3(p.g.nblk), dim3(256), 0, stream, x, dy, p.g, mean, invstd, gamma,
                       beta, 0, relu, mask_y, rows, gslots, counters, groups, fo);
    launch_apply_bwd<decltype(f), decltype(v)::value, false>(p, a, nullptr, o, stream);
  });
  FV2P_LAUNCH_CHECK();
  return 0;
}
