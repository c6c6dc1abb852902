// BatchNorm2d on NCHW maps: what the fp32 kernels (batchnorm2d.hip) and the 16-bit kernels (batchnorm2d_h.hip) share - the grid of
// (sample, channel, chunk of the plane) workgroups, the fixed-order fold of the per-workgroup fp64 partials, the ONE expression of the
// layer's value at an element, and the workspace layout.
#pragma once
#include "common.hpp"
#include "bn_fold.hpp"

namespace fv2p {

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

// 0, or the reason the shape cannot be launched
static const char* bn2d_geom(int64_t n, int c, int64_t hw, Bn2dGeom* g) {
  g->n = n; g->c = c; g->hw = hw;
  g->chunks = ceil_div(hw, kBn2dChunk);
  if (n > INT32_MAX / g->chunks) return "partials per channel";
  g->parts = static_cast<int>(n * g->chunks);
  if (static_cast<int64_t>(g->parts) * c > kBn2dMaxGrid) return "workgroups";
  g->count = static_cast<double>(n) * static_cast<double>(hw);
  return nullptr;
}
static unsigned bn2d_grid(const Bn2dGeom& g) { return static_cast<unsigned>(static_cast<int64_t>(g.parts) * g.c); }

struct Bn2dWs {
  double* partial;
  long long* nbt_copy;
};
template <typename C>
static Bn2dWs bn2d_ws(C& cv, const Bn2dGeom& g) {
  Bn2dWs w;
  w.partial = cv.template take<double>(static_cast<size_t>(g.parts) * g.c * 2);
  w.nbt_copy = cv.template take<long long>(1);
  return w;
}

}  // namespace fv2p
