// Voxel R-CNN RoI-grid pooling (NeighborVoxelSAModuleMSG between mlps_in and mlps_out, pool_method 'max_pool') as one op without the
// grouped (M, C, S) tensor (DESIGN: "Voxel pooling").  Per grouper, with F [n][c] the mlps_in rows, idx [m][s] GLOBAL rows of the
// voxel query, d[i][j] = xyz[idx[i][j]] - new_xyz[i] (fp32; zero for an empty query) and W [c][3] the Conv2d(3, c, 1) weight:
//
//   position branch z = W d is linear in d, so the statistics of its training-mode BatchNorm2d over the n_pos = m * s positions
//   follow from nine sums that do not depend on the channel, m1 = sum d and m2 = sum d d^T:
//     mean_c = w_c . m1 / n_pos      var_c = w_c^T m2 w_c / n_pos - mean_c^2  (biased, clamped at 0)      invstd_c = 1 / sqrt(var_c + eps)
//     a_c = gamma_c invstd_c w_c     b_c = beta_c - gamma_c invstd_c mean_c
//     out[i][c] = max_j relu(F[idx[i][j]][c] + a_c . d[i][j] + b_c)                                   (empty query: relu(b_c))
//   backward, j* the winning sample, g = grad_out * [out > 0], sg_c = sum_i g, sgd_c = sum_i g d[i][j*]:
//     grad_F[idx[i][j*]][c] += g      dbeta_c = sg_c      dgamma_c = invstd_c (w_c . sgd_c - mean_c sg_c)
//     dW_c = gamma_c invstd_c (sgd_c - (sg_c / n_pos) m1 - (dgamma_c / n_pos) invstd_c (m2 w_c - mean_c m1))
//     eval mode (running statistics): dW_c = gamma_c invstd_c sgd_c
//
// Launches.  forward: moments (fixed blocks of kVpBlock queries, fp64, one row of 9 partials per block) -> fold (one workgroup:
// block order, per-channel coefficients in fp64, running statistics through bn_move_running) -> pool.  backward: route (g, the
// destination element of every (query, channel), per-block fp64 partials of sg / sgd) -> fold (closed forms above) -> zero fill and
// fv2p_scatter_add with one channel per entry.  Every sum across workgroups is a row of partials that a LATER launch folds in block
// order: no float atomics, no workgroup waits for another, every output is bit-identical from run to run.
// An idx entry outside [0, n) is a row of zeros of F AND of xyz (d = 0 - new_xyz[i]) and receives no gradient, the rule of
// sa_fused.hip: no input makes a kernel read or write outside its buffers.
//
// Row formats.  pool and route - the two kernels that touch F, out, grad_out and the staged g - are written once and instantiated for
// F32, Fmt16<H16> and Fmt16<B16> (bn_fmt.hpp): the *_h entry points take float16 / bfloat16 rows (F, out, grad_out, grad_F) beside
// the same fp32 coordinates and parameters.  A 16-bit row is widened on load; the sum, the ReLU, the maximum and the arg-max byte are
// fp32 exactly as in the fp32 instance, out is rounded to nearest even ONCE at the store, the ReLU mask of the backward reads the
// stored output widened, g (grad_out or 0: exact) is staged in the rows' format and grad_F goes through scatter_add_h (the fp32
// association of fv2p_scatter_add, one rounding).  moments and the two folds never see F and are shared.
#include "common.hpp"
#include "bn_fold.hpp"
#include "bn_fmt.hpp"
#include <type_traits>

namespace fv2p {

constexpr int kVpBlock = 64;        // queries of one partial-sum block (moments and route): fv2p_voxel_pool_blocks
constexpr int kVpSub = 4;           // moments: lanes per query, interleaved samples
constexpr int kVpEntries = 2048;    // pool: (query, sample) entries of one workgroup in LDS
constexpr int kVpHead = 16;         // saved: m1 (3), m2 (xx xy xz yy yz zz), padding; then mean [c], invstd [c] - all fp64
constexpr int kVpFoldSub = 28;      // forward fold: lanes per moment column (9 x 28 <= 256)

struct VpEntry { float dx, dy, dz; int row; };   // row: the F row, -1 for an empty query or an index out of range

__device__ __forceinline__ VpEntry vp_entry(const float* __restrict__ xyz, const float* __restrict__ q, int r, bool empty, int64_t n) {
  VpEntry e;
  if (empty) { e.dx = 0.f; e.dy = 0.f; e.dz = 0.f; e.row = -1; return e; }
  const bool in = r >= 0 && static_cast<int64_t>(r) < n;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (in) { const float* p = xyz + static_cast<int64_t>(r) * 3; px = p[0]; py = p[1]; pz = p[2]; }
  e.dx = px - q[0]; e.dy = py - q[1]; e.dz = pz - q[2];
  e.row = in ? r : -1;
  return e;
}

// ---- 1. moments: block b takes queries [b * kVpBlock, ...), kVpSub lanes per query walk interleaved samples in ascending order;
// fixed tree over the 256 lanes; part[b][9] with plain stores ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void vp_moments_k(int64_t m, int s, int64_t n, const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                    const int* __restrict__ idx, const unsigned char* __restrict__ empty,
                                                    double* __restrict__ part) {
  __shared__ double red[9][256];
  const int tid = threadIdx.x;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kVpBlock + tid / kVpSub;
  const int sub = tid % kVpSub;
  double a[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) a[k] = 0.0;
  if (i < m && !empty[i]) {
    const float* q = new_xyz + i * 3;
    const int* row = idx + i * s;
#pragma unroll 4
    for (int j = sub; j < s; j += kVpSub) {
      const VpEntry e = vp_entry(xyz, q, row[j], false, n);
      const double x = e.dx, y = e.dy, z = e.dz;
      a[0] += x; a[1] += y; a[2] += z;
      a[3] += x * x; a[4] += x * y; a[5] += x * z; a[6] += y * y; a[7] += y * z; a[8] += z * z;
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) red[k][tid] = a[k];
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int k = 0; k < 9; ++k) red[k][tid] += red[k][tid + w];
    }
    __syncthreads();
  }
  if (tid < 9) part[static_cast<int64_t>(blockIdx.x) * 9 + tid] = red[tid][0];
}

// ---- 2. forward fold (one workgroup): the partial rows in block order (kVpFoldSub interleaved lanes per column, then an ordered
// fold), mean / var / invstd and the coefficients a_c, b_c of every channel in fp64, running statistics with torch's semantics.
// Eval mode: the coefficients from the running statistics, nothing else is touched. ------------------------------------------------
__global__ __launch_bounds__(256) void vp_fold_fwd_k(int64_t blocks, int c, long long n_pos, int training, const double* __restrict__ part,
                                                     const float* __restrict__ w, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float* running_mean, float* running_var, long long* nbt, float momentum, float eps,
                                                     double* __restrict__ saved, float* __restrict__ coef) {
  __shared__ double red[9][kVpFoldSub];
  __shared__ double mom[9];
  const int tid = threadIdx.x;
  if (training) {
    const int col = tid % 9, sub = tid / 9;
    if (sub < kVpFoldSub) {
      double a = 0.0;
      for (int64_t b = sub; b < blocks; b += kVpFoldSub) a += part[b * 9 + col];
      red[col][sub] = a;
    }
    __syncthreads();
    if (tid < 9) {
      double a = 0.0;
      for (int q = 0; q < kVpFoldSub; ++q) a += red[tid][q];
      mom[tid] = a;
    }
    __syncthreads();
  } else if (tid < 9) {
    mom[tid] = 0.0;
  }
  if (tid < kVpHead) saved[tid] = tid < 9 && training ? mom[tid] : 0.0;
  if (tid < c) {
    const double wx = w[3 * tid], wy = w[3 * tid + 1], wz = w[3 * tid + 2];
    const double g = gamma[tid], bt = beta[tid];
    double mean, invstd;
    if (training) {
      const double nn = static_cast<double>(n_pos);
      mean = (wx * mom[0] + wy * mom[1] + wz * mom[2]) / nn;
      const double e2 = (wx * (wx * mom[3] + wy * mom[4] + wz * mom[5]) + wy * (wx * mom[4] + wy * mom[6] + wz * mom[7]) +
                         wz * (wx * mom[5] + wy * mom[7] + wz * mom[8])) / nn;
      double var = e2 - mean * mean;
      if (var < 0.0) var = 0.0;
      invstd = 1.0 / sqrt(var + static_cast<double>(eps));
      if (running_mean) bn_move_running<F32>(mean, var, n_pos, running_mean, running_var, 0, momentum, nbt, tid);
    } else {
      mean = running_mean[tid];
      invstd = 1.0 / sqrt(static_cast<double>(running_var[tid]) + static_cast<double>(eps));
    }
    saved[kVpHead + tid] = mean;
    saved[kVpHead + c + tid] = invstd;
    const double gi = g * invstd;
    coef[4 * tid + 0] = static_cast<float>(gi * wx);
    coef[4 * tid + 1] = static_cast<float>(gi * wy);
    coef[4 * tid + 2] = static_cast<float>(gi * wz);
    coef[4 * tid + 3] = static_cast<float>(bt - gi * mean);
  }
  // momentum=None: every channel above read *nbt; the bump comes after all of them (c <= 128: one workgroup)
  __syncthreads();
  if (training && tid == 0 && running_mean && nbt) *nbt += 1;
}

// ---- 3. pool: c / 4 lanes per query, each owns 4 consecutive channels; qpw queries per workgroup (the lanes that do not fill a
// query are masked: c = 12 leaves one of 256).  The (d, row) entries of the workgroup's queries are formed once, into LDS rows
// padded by one 16-byte slot (queries s slots apart would all read one bank group); the F rows come by 16-byte gathers (8-byte ones
// of 16-bit rows), four in flight per lane. ------------------------------------------------------------------------------------------
// 4 consecutive channels of a row in format R as fp32: one 16-byte (F32) or one 8-byte (Fmt16) access
template <class R>
__device__ __forceinline__ float4 vp_load4(const typename R::elem* p) {
  if constexpr (sizeof(typename R::elem) == 4) {
    return *reinterpret_cast<const float4*>(p);
  } else {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
    return make_float4(R::widen(static_cast<u16>(q.x & 0xffffu)), R::widen(static_cast<u16>(q.x >> 16)),
                       R::widen(static_cast<u16>(q.y & 0xffffu)), R::widen(static_cast<u16>(q.y >> 16)));
  }
}
template <class R>
__device__ __forceinline__ void vp_store4(typename R::elem* p, const float4& v) {   // Fmt16: the one rounding, nearest even
  if constexpr (sizeof(typename R::elem) == 4) {
    *reinterpret_cast<float4*>(p) = v;
  } else {
    *reinterpret_cast<uint2*>(p) = make_uint2(static_cast<unsigned>(R::narrow(v.x)) | (static_cast<unsigned>(R::narrow(v.y)) << 16),
                                              static_cast<unsigned>(R::narrow(v.z)) | (static_cast<unsigned>(R::narrow(v.w)) << 16));
  }
}

__device__ __forceinline__ void vp_take(float g, const float4& a, const float4& e, int j, float* best, int* bj) {
  const float v = g + fmaf(a.x, e.x, fmaf(a.y, e.y, fmaf(a.z, e.z, a.w)));
  const float r = v < 0.f ? 0.f : v;            // relu; a NaN stays
  if (r > *best || r != r) { *best = r; *bj = j; }   // max_pool2d's scan: strict >, a NaN candidate always enters
}

template <class R>
__global__ __launch_bounds__(256) void vp_pool_k(int64_t m, int s, int c, int64_t n, int qpw, const typename R::elem* __restrict__ f,
                                                 const float* __restrict__ xyz, const float* __restrict__ new_xyz, const int* __restrict__ idx,
                                                 const unsigned char* __restrict__ empty, const float* __restrict__ coef,
                                                 typename R::elem* __restrict__ out, unsigned char* __restrict__ arg) {
  extern __shared__ float4 vp_ent[];   // [qpw][s + 1]
  const int tid = threadIdx.x, L = c >> 2, ld = s + 1;
  const int64_t q0 = static_cast<int64_t>(blockIdx.x) * qpw;
  const int nq = static_cast<int>(m - q0 < qpw ? m - q0 : qpw);
  for (int t = tid; t < nq * s; t += 256) {
    const int q = t / s, j = t - q * s;
    const int64_t i = q0 + q;
    const VpEntry e = vp_entry(xyz, new_xyz + i * 3, idx[i * s + j], empty[i] != 0, n);
    vp_ent[q * ld + j] = make_float4(e.dx, e.dy, e.dz, __int_as_float(e.row));
  }
  __syncthreads();
  const int q = tid / L, l = tid - q * L;
  if (q >= nq) return;
  const float4* cf = reinterpret_cast<const float4*>(coef) + 4 * l;
  const float4 a0 = cf[0], a1 = cf[1], a2 = cf[2], a3 = cf[3];
  float best[4];
  int bj[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { best[k] = -INFINITY; bj[k] = 0; }
  const float4* ent = vp_ent + q * ld;
  const typename R::elem* fl = f + 4 * l;
  for (int j0 = 0; j0 < s; j0 += 4) {
    float4 e[4], g[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      e[u] = ent[j0 + u < s ? j0 + u : s - 1];
      const int row = __float_as_int(e[u].w);
      g[u] = row >= 0 ? vp_load4<R>(fl + static_cast<int64_t>(row) * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (j0 + u < s) {
        vp_take(g[u].x, a0, e[u], j0 + u, &best[0], &bj[0]);
        vp_take(g[u].y, a1, e[u], j0 + u, &best[1], &bj[1]);
        vp_take(g[u].z, a2, e[u], j0 + u, &best[2], &bj[2]);
        vp_take(g[u].w, a3, e[u], j0 + u, &best[3], &bj[3]);
      }
  }
  const int64_t o = (q0 + q) * c + 4 * l;
  vp_store4<R>(out + o, make_float4(best[0], best[1], best[2], best[3]));
  if (arg) *reinterpret_cast<uchar4*>(arg + o) = make_uchar4(static_cast<unsigned char>(bj[0]), static_cast<unsigned char>(bj[1]),
                                                             static_cast<unsigned char>(bj[2]), static_cast<unsigned char>(bj[3]));
}

// ---- 4. route: block b takes queries [b * kVpBlock, ...), c / 4 lanes per query in passes of 256 / (c / 4) queries.  Per
// (query, channel): g = grad_out * [out > 0] (out as stored, widened; g staged in the rows' format: exact), the destination element idx[i][arg] * c + channel of grad_F (-1: masked, empty query,
// row out of range), and the lane's fp64 sums of g and g * d[i][arg] in pass order; the block's lanes are then folded in lane order
// into part[b][c][4]. ---------------------------------------------------------------------------------------------------------------
template <class R>
__global__ __launch_bounds__(256) void vp_route_k(int64_t m, int s, int c, int64_t n, const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                  const int* __restrict__ idx, const unsigned char* __restrict__ empty,
                                                  const typename R::elem* __restrict__ out, const unsigned char* __restrict__ arg,
                                                  const typename R::elem* __restrict__ gy, typename R::elem* __restrict__ gbuf,
                                                  int* __restrict__ dst, double* __restrict__ part) {
  __shared__ double red[256][17];
  const int tid = threadIdx.x, L = c >> 2, qpp = 256 / L;
  const int q = tid / L, l = tid - q * L;
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kVpBlock;
  if (q < qpp) {
    for (int qq = q; qq < kVpBlock; qq += qpp) {
      const int64_t i = base + qq;
      if (i >= m) break;
      const int64_t o = i * c + 4 * l;
      const float4 ov = vp_load4<R>(out + o), gv = vp_load4<R>(gy + o);
      const uchar4 av = *reinterpret_cast<const uchar4*>(arg + o);
      const float oo[4] = {ov.x, ov.y, ov.z, ov.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w};
      const int aa[4] = {av.x, av.y, av.z, av.w};
      const bool em = empty[i] != 0;
      float g[4];
      int d[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool live = oo[k] > 0.f;
        g[k] = live ? gg[k] : 0.f;
        d[k] = -1;
        if (live) {
          const int j = aa[k] < s ? aa[k] : s - 1;
          const VpEntry e = vp_entry(xyz, new_xyz + i * 3, em ? 0 : idx[i * s + j], em, n);
          const double gd = g[k];
          acc[4 * k + 0] += gd;
          acc[4 * k + 1] += gd * static_cast<double>(e.dx);
          acc[4 * k + 2] += gd * static_cast<double>(e.dy);
          acc[4 * k + 3] += gd * static_cast<double>(e.dz);
          if (e.row >= 0) d[k] = static_cast<int>(static_cast<int64_t>(e.row) * c + 4 * l + k);   // n * c < 2^31 - 1: checked by the caller
        }
      }
      if (gbuf) {
        vp_store4<R>(gbuf + o, make_float4(g[0], g[1], g[2], g[3]));
        *reinterpret_cast<int4*>(dst + o) = make_int4(d[0], d[1], d[2], d[3]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) red[tid][k] = acc[k];
  __syncthreads();
  for (int o = tid; o < c * 4; o += 256) {
    const int ch = o >> 2, k = o & 3, ll = ch >> 2, col = (ch & 3) * 4 + k;
    double a = 0.0;
    for (int p = 0; p < qpp; ++p) a += red[p * L + ll][col];
    part[static_cast<int64_t>(blockIdx.x) * c * 4 + o] = a;
  }
}

// ---- 5. backward fold (one workgroup): the partial rows in block order, then the closed forms in fp64 ------------------------------
__global__ __launch_bounds__(256) void vp_fold_bwd_k(int64_t blocks, int c, long long n_pos, int training, const double* __restrict__ part,
                                                     const float* __restrict__ w, const float* __restrict__ gamma, const double* __restrict__ saved,
                                                     float* __restrict__ gw, float* __restrict__ ggamma, float* __restrict__ gbeta) {
  __shared__ double tot[128 * 4];
  const int tid = threadIdx.x;
  for (int o = tid; o < c * 4; o += 256) {
    double a = 0.0;
#pragma unroll 8
    for (int64_t b = 0; b < blocks; ++b) a += part[b * c * 4 + o];
    tot[o] = a;
  }
  __syncthreads();
  if (tid >= c) return;
  const double sg = tot[4 * tid], sx = tot[4 * tid + 1], sy = tot[4 * tid + 2], sz = tot[4 * tid + 3];
  const double wx = w[3 * tid], wy = w[3 * tid + 1], wz = w[3 * tid + 2], g = gamma[tid];
  const double mean = saved[kVpHead + tid], invstd = saved[kVpHead + c + tid];
  const double dgamma = invstd * (wx * sx + wy * sy + wz * sz - mean * sg);
  if (gbeta) gbeta[tid] = static_cast<float>(sg);
  if (ggamma) ggamma[tid] = static_cast<float>(dgamma);
  if (!gw) return;
  double dx = sx, dy = sy, dz = sz;
  if (training) {
    const double nn = static_cast<double>(n_pos);
    const double m1x = saved[0], m1y = saved[1], m1z = saved[2];
    const double xx = saved[3], xy = saved[4], xz = saved[5], yy = saved[6], yz = saved[7], zz = saved[8];
    const double k1 = sg / nn, k2 = dgamma / nn * invstd;
    dx = sx - k1 * m1x - k2 * (xx * wx + xy * wy + xz * wz - mean * m1x);
    dy = sy - k1 * m1y - k2 * (xy * wx + yy * wy + yz * wz - mean * m1y);
    dz = sz - k1 * m1z - k2 * (xz * wx + yz * wy + zz * wz - mean * m1z);
  }
  const double gi = g * invstd;
  gw[3 * tid] = static_cast<float>(gi * dx);
  gw[3 * tid + 1] = static_cast<float>(gi * dy);
  gw[3 * tid + 2] = static_cast<float>(gi * dz);
}

static bool vp_ok(int64_t m, int s, int c) {
  return c % 4 == 0 && c >= 4 && c <= 128 && s >= 1 && s <= 64 && m >= 1 && m * s < (1ll << 31);
}
static int64_t vp_blocks(int64_t m) { return m < 1 ? 0 : ceil_div(m, kVpBlock); }
// queries per pool workgroup: what 256 lanes hold at c / 4 lanes each, and what the LDS entries hold
static int vp_qpw(int s, int c) {
  const int a = 256 / (c / 4), b = kVpEntries / s;
  return a < b ? a : b;
}
static bool vp_bwd_ok(int64_t m, int s, int c, int64_t n) {   // the scatter-add's 32-bit entry and destination numbers
  return vp_ok(m, s, c) && n >= 1 && m * c < (1ll << 31) && n * c < (1ll << 31) - 1;
}

struct VpFwdWs { double* part; float* coef; };
template <class Cv> static VpFwdWs vp_fwd_ws(Cv& cv, int64_t m, int c) {
  VpFwdWs w;
  w.part = cv.template take<double>(static_cast<size_t>(vp_blocks(m)) * 9);
  w.coef = cv.template take<float>(static_cast<size_t>(c) * 4);
  return w;
}
// backward workspace.  fp32: part, g, dst, the scatter-add's own.  16-bit: g (2 bytes per cell) comes LAST and the size is the
// unpadded end of it, so that the query is 2 m c bytes below the fp32 one at least, whatever the 256-byte padding of the regions does.
template <class R> struct VpBwdWs { double* part; typename R::elem* g; int* dst; void* sws; size_t sws_bytes; size_t bytes; };
template <class R, class Cv> static VpBwdWs<R> vp_bwd_ws(Cv& cv, int64_t m, int c) {
  constexpr bool k16 = sizeof(typename R::elem) == 2;
  VpBwdWs<R> w;
  w.part = cv.template take<double>(static_cast<size_t>(vp_blocks(m)) * c * 4);
  if constexpr (!k16) w.g = cv.template take<typename R::elem>(static_cast<size_t>(m) * c);
  w.dst = cv.template take<int>(static_cast<size_t>(m) * c);
  w.sws_bytes = fv2p_scatter_add_ws_bytes(m * c, 1);
  w.sws = cv.template take<char>(w.sws_bytes);
  if constexpr (k16) w.g = cv.template take<typename R::elem>(static_cast<size_t>(m) * c);
  w.bytes = k16 ? cv.off : align_up(cv.off);
  return w;
}

// what a lane's access of 4 channels needs of the row pointers: 16 bytes (fp32 rows) or 8 (16-bit rows)
template <class R> constexpr uintptr_t kVpAlign = 4 * sizeof(typename R::elem);
template <class R> static bool vp_aligned(const void* a, const void* b, const unsigned char* arg) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & (kVpAlign<R> - 1)) == 0 && (reinterpret_cast<uintptr_t>(arg) & 3) == 0;
}

template <class R>
static int vp_forward(const char* who, const typename R::elem* f, const float* xyz, const float* new_xyz, const int* idx, const unsigned char* empty,
                      int64_t n, int64_t m, int s, int c, const float* w, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, int64_t* num_batches_tracked, float momentum, float eps, int training, typename R::elem* out,
                      unsigned char* arg, double* saved, void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  FV2P_REQUIRE(vp_ok(m, s, c), FV2P_ELIMIT, "%s: m %lld, s %d, c %d outside fv2p_voxel_pool_supported", who, static_cast<long long>(m), s, c);
  FV2P_REQUIRE(n >= 1 && n < (1ll << 31), FV2P_EINVAL, "%s: n %lld rows", who, static_cast<long long>(n));
  FV2P_REQUIRE(f && xyz && new_xyz && idx && empty && w && gamma && beta && out && saved && ws, FV2P_EINVAL, "%s: null pointer", who);
  FV2P_REQUIRE(training || (running_mean && running_var), FV2P_EINVAL, "%s: eval mode needs the running statistics", who);
  FV2P_REQUIRE(!training || m * s >= 2, FV2P_EINVAL, "%s: batch statistics of a single position", who);
  FV2P_REQUIRE(vp_aligned<R>(f, out, arg), FV2P_EINVAL, "%s: F and out must be %d-byte aligned, arg 4-byte aligned", who, static_cast<int>(kVpAlign<R>));
  FV2P_REQUIRE(ws_bytes >= fv2p_voxel_pool_ws_bytes(m, s, c), FV2P_EWORKSPACE, "%s: workspace too small", who);
  hipStream_t st = static_cast<hipStream_t>(stream);
  Carver cv(ws, ws_bytes);
  const VpFwdWs wk = vp_fwd_ws(cv, m, c);
  const int64_t blocks = vp_blocks(m);
  if (training)
    hipLaunchKernelGGL(vp_moments_k, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, st, m, s, n, xyz, new_xyz, idx, empty, wk.part);
  hipLaunchKernelGGL(vp_fold_fwd_k, dim3(1), dim3(256), 0, st, blocks, c, static_cast<long long>(m * s), training ? 1 : 0, wk.part, w, gamma, beta,
                     running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked), momentum, eps, saved, wk.coef);
  const int qpw = vp_qpw(s, c);
  const size_t lds = static_cast<size_t>(qpw) * (s + 1) * sizeof(float4);
  hipLaunchKernelGGL((vp_pool_k<R>), dim3(static_cast<unsigned>(ceil_div(m, qpw))), dim3(256), lds, st, m, s, c, n, qpw, f, xyz, new_xyz, idx, empty,
                     wk.coef, out, arg);
  FV2P_LAUNCH_CHECK();
  return 0;
}

template <class R>
static int vp_backward(const char* who, const float* xyz, const float* new_xyz, const int* idx, const unsigned char* empty, int64_t n, int64_t m,
                       int s, int c, const float* w, const float* gamma, const typename R::elem* out, const unsigned char* arg,
                       const double* saved, const typename R::elem* grad_out, int training, typename R::elem* grad_f, float* grad_w,
                       float* grad_gamma, float* grad_beta, void* ws, size_t ws_bytes, fv2p_stream_t stream) {
  FV2P_REQUIRE(vp_ok(m, s, c), FV2P_ELIMIT, "%s: m %lld, s %d, c %d outside fv2p_voxel_pool_supported", who, static_cast<long long>(m), s, c);
  FV2P_REQUIRE(vp_bwd_ok(m, s, c, n), FV2P_ELIMIT, "%s: m * c or n * c reaches 2^31 (n %lld)", who, static_cast<long long>(n));
  FV2P_REQUIRE(xyz && new_xyz && idx && empty && w && gamma && out && arg && saved && grad_out && ws, FV2P_EINVAL, "%s: null pointer", who);
  FV2P_REQUIRE(vp_aligned<R>(out, grad_out, arg), FV2P_EINVAL, "%s: out and grad_out must be %d-byte aligned, arg 4-byte aligned", who,
               static_cast<int>(kVpAlign<R>));
  Sizer sz;
  FV2P_REQUIRE(ws_bytes >= vp_bwd_ws<R>(sz, m, c).bytes, FV2P_EWORKSPACE, "%s: workspace too small", who);
  if (!grad_f && !grad_w && !grad_gamma && !grad_beta) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Carver cv(ws, ws_bytes);
  const VpBwdWs<R> wk = vp_bwd_ws<R>(cv, m, c);
  const int64_t blocks = vp_blocks(m);
  hipLaunchKernelGGL((vp_route_k<R>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, st, m, s, c, n, xyz, new_xyz, idx, empty, out, arg, grad_out,
                     grad_f ? wk.g : nullptr, wk.dst, wk.part);
  if (grad_w || grad_gamma || grad_beta)
    hipLaunchKernelGGL(vp_fold_bwd_k, dim3(1), dim3(256), 0, st, blocks, c, static_cast<long long>(m * s), training ? 1 : 0, wk.part, w, gamma, saved,
                       grad_w, grad_gamma, grad_beta);
  FV2P_LAUNCH_CHECK();
  if (!grad_f) return 0;
  if constexpr (sizeof(typename R::elem) == 4) {
    FV2P_HIP(hipMemsetAsync(grad_f, 0, static_cast<size_t>(n) * c * sizeof(float), st));
    return fv2p_scatter_add(m * c, 1, n * c, wk.dst, nullptr, nullptr, wk.g, 1, grad_f, wk.sws, wk.sws_bytes, stream);
  } else {   // zero-fills grad_f itself; every element's fp32 total is rounded once.  The format's code follows from R.
    constexpr int dtype = std::is_same_v<R, Fmt16<H16>> ? FV2P_DT_F16 : FV2P_DT_BF16;
    static_assert(std::is_same_v<R, Fmt16<H16>> || std::is_same_v<R, Fmt16<B16>>, "a 16-bit row format");
    return scatter_add_h(m * c, 1, n * c, wk.dst, nullptr, nullptr, wk.g, 1, grad_f, dtype, wk.sws, wk.sws_bytes, st);
  }
}

}  // namespace fv2p
using namespace fv2p;

extern "C" int fv2p_voxel_pool_supported(int64_t m, int s, int c) { return vp_ok(m, s, c) ? 1 : 0; }

extern "C" int fv2p_voxel_pool_blocks(int64_t m) { return static_cast<int>(vp_blocks(m < (1ll << 31) ? m : (1ll << 31) - 1)); }

extern "C" size_t fv2p_voxel_pool_saved_bytes(int c) { return c >= 1 ? (kVpHead + 2 * static_cast<size_t>(c)) * sizeof(double) : 0; }

extern "C" size_t fv2p_voxel_pool_ws_bytes(int64_t m, int s, int c) {
  if (!vp_ok(m, s, c)) return 0;
  Sizer sz;
  vp_fwd_ws(sz, m, c);
  return sz.bytes();
}

extern "C" size_t fv2p_voxel_pool_backward_ws_bytes(int64_t m, int s, int c, int64_t n) {
  if (!vp_bwd_ok(m, s, c, n)) return 0;
  Sizer sz;
  return vp_bwd_ws<F32>(sz, m, c).bytes;
}

extern "C" size_t fv2p_voxel_pool_backward_h_ws_bytes(int64_t m, int s, int c, int64_t n) {   // the same for both 16-bit formats
  if (!vp_bwd_ok(m, s, c, n)) return 0;
  Sizer sz;
  return vp_bwd_ws<Fmt16<H16>>(sz, m, c).bytes;
}

extern "C" int fv2p_voxel_pool_forward(const float* f, const float* xyz, const float* new_xyz, const int* idx, const unsigned char* empty,
                                       int64_t n, int64_t m, int s, int c, const float* w, const float* gamma, const float* beta,
                                       float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                                       int training, float* out, unsigned char* arg, double* saved, void* ws, size_t ws_bytes,
                                       fv2p_stream_t stream) {
  return vp_forward<F32>("fv2p_voxel_pool_forward", f, xyz, new_xyz, idx, empty, n, m, s, c, w, gamma, beta, running_mean, running_var,
                         num_batches_tracked, momentum, eps, training, out, arg, saved, ws, ws_bytes, stream);
}

extern "C" int fv2p_voxel_pool_forward_h(const void* f, const float* xyz, const float* new_xyz, const int* idx, const unsigned char* empty,
                                         int64_t n, int64_t m, int s, int c, const float* w, const float* gamma, const float* beta,
                                         float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                                         int training, void* out, unsigned char* arg, double* saved, void* ws, size_t ws_bytes, int dtype,
                                         fv2p_stream_t stream) {
  FV2P_DT16_OK("fv2p_voxel_pool_forward_h", dtype);
  if (dtype == FV2P_DT_F16)
    return vp_forward<Fmt16<H16>>("fv2p_voxel_pool_forward_h", static_cast<const u16*>(f), xyz, new_xyz, idx, empty, n, m, s, c, w, gamma, beta,
                                  running_mean, running_var, num_batches_tracked, momentum, eps, training, static_cast<u16*>(out), arg, saved,
                                  ws, ws_bytes, stream);
  return vp_forward<Fmt16<B16>>("fv2p_voxel_pool_forward_h", static_cast<const u16*>(f), xyz, new_xyz, idx, empty, n, m, s, c, w, gamma, beta,
                                running_mean, running_var, num_batches_tracked, momentum, eps, training, static_cast<u16*>(out), arg, saved, ws,
                                ws_bytes, stream);
}

extern "C" int fv2p_voxel_pool_backward(const float* xyz, const float* new_xyz, const int* idx, const unsigned char* empty, int64_t n,
                                        int64_t m, int s, int c, const float* w, const float* gamma, const float* out,
                                        const unsigned char* arg, const double* saved, const float* grad_out, int training, float* grad_f,
                                        float* grad_w, float* grad_gamma, float* grad_beta, void* ws, size_t ws_bytes,
                                        fv2p_stream_t stream) {
  return vp_backward<F32>("fv2p_voxel_pool_backward", xyz, new_xyz, idx, empty, n, m, s, c, w, gamma, out, arg, saved, grad_out, training, grad_f,
                          grad_w, grad_gamma, grad_beta, ws, ws_bytes, stream);
}

extern "C" int fv2p_voxel_pool_backward_h(const float* xyz, const float* new_xyz, const int* idx, const unsigned char* empty, int64_t n,
                                          int64_t m, int s, int c, const float* w, const float* gamma, const void* out,
                                          const unsigned char* arg, const double* saved, const void* grad_out, int training, void* grad_f,
                                          float* grad_w, float* grad_gamma, float* grad_beta, void* ws, size_t ws_bytes, int dtype,
                                          fv2p_stream_t stream) {
  FV2P_DT16_OK("fv2p_voxel_pool_backward_h", dtype);
  if (dtype == FV2P_DT_F16)
    return vp_backward<Fmt16<H16>>("fv2p_voxel_pool_backward_h", xyz, new_xyz, idx, empty, n, m, s, c, w, gamma, static_cast<const u16*>(out), arg,
                                   saved, static_cast<const u16*>(grad_out), training, static_cast<u16*>(grad_f), grad_w, grad_gamma, grad_beta,
                                   ws, ws_bytes, stream);
  return vp_backward<Fmt16<B16>>("fv2p_voxel_pool_backward_h", xyz, new_xyz, idx, empty, n, m, s, c, w, gamma, static_cast<const u16*>(out), arg,
                                 saved, static_cast<const u16*>(grad_out), training, static_cast<u16*>(grad_f), grad_w, grad_gamma, grad_beta,
                                 ws, ws_bytes, stream);
}
