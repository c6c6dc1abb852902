// A1 — hashed first-come voxeliser (replaces the numba kernel
// pcdet/datasets/processor/voxel_generator.py:136-207 of the reference).
//
// The reference is a sequential loop over points with a dense [Z,Y,X] int map (360 MB per
// call at KITTI resolution).  Here the map is an open-addressing hash table of packed
// {flat voxel key : 40, first point index : 24} words:
//   1. insert   : atomicMin on the packed word keeps, per voxel, the smallest point index;
//   2. order    : a point is "first" iff it is that minimum; an exclusive scan over the
//                 first-flags gives every voxel its reference id (= order of first touch);
//   3. cut-off  : the first-flagged point whose id == max_voxels is where the reference
//                 loop `break`s (voxel_generator.py:198-199); later points are dropped;
//   4. slots    : kept points are keyed (voxel id, point index) and radix-sorted on the
//                 voxel-id bits (stable, so input order inside a voxel survives); the slot
//                 of a point is its sorted position minus the voxel's start offset.
// All integer outputs are therefore bit-identical to the sequential loop.
//
// One pipeline, two policies.  Steps 1, 2 and 4 are the same code for one cloud (VoxOne) and for a stacked batch of B unequal clouds in
// one point buffer (VoxStacked): vox_insert and vox_mark_first are templated on the policy, one workspace layout (vox_carve) and one
// host tail (vox_sort_fill) serve both.  The policy says what sample a point belongs to - with VoxOne nothing, the key is the flat
// cell; with VoxStacked the key is sample * grid volume + flat cell, so that atomicMin keeps the first point of every (sample, voxel).
// Step 3 is where the routes really differ and stays two sets of kernels:
//   one cloud : vox_assign finds the one break point, vox_finalize_scalars the voxel count, vox_words keys the kept points;
//   stacked   : one scan of the first-flags over the whole buffer (n + 1 entries: rank[n] = all firsts), a first point's rank inside its
//               sample is rank[i] - rank[off[b]].  Per sample, the break point is the first-flagged point of rank max_voxels (a binary
//               search over the monotone rank[]: the smallest i of the sample with rank[i + 1] > rank[off[b]] + max_voxels); the
//               sample's later points are dropped, other samples are unaffected.  Sample b keeps M_b = min(distinct voxels,
//               max_voxels) voxels, its output rows start at base[b] = sum of M_a over a < b (vox_stack_bases: one workgroup, the only
//               per-sample pass); vox_stack_words keys the kept points by output row and writes the rows' (b, z, y, x).
// The number of launches of the stacked route does not depend on B (the offsets reach the device as kernel arguments, 256 per launch).
#include "common.hpp"
#include <cmath>
#include <cstring>
#include <vector>

namespace fv2p {

struct VoxGeom {
  float vs[3];   // voxel size x,y,z
  float lo[3];   // range min x,y,z
  int grid[3];   // cells x,y,z
};
static VoxGeom vox_geom(const float voxel_size[3], const float range_lo[3], const int grid[3]) {
  VoxGeom g;
  for (int j = 0; j < 3; ++j) { g.vs[j] = voxel_size[j]; g.lo[j] = range_lo[j]; g.grid[j] = grid[j]; }
  return g;
}

// The cell (x, y, z) of a point; false when it lies outside the grid (NaN coordinates too).  The one line every output's bit-exactness
// rests on: fp32 subtract, then fp32 divide, then floor, as voxel_generator.py:188 (no reciprocal, no fma: the file is built with
// -ffp-contract=off for the host and the device).  c[] is meaningful only when the point is inside.
__host__ __device__ __forceinline__ bool vox_cell(const float* __restrict__ p, const VoxGeom& g, int c[3]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float f = floorf((p[j] - g.lo[j]) / g.vs[j]);
    if (!(f >= 0.0f) || f >= static_cast<float>(g.grid[j])) ok = false;  // (:189-191) NaN -> dropped
    c[j] = static_cast<int>(f);
  }
  return ok;
}
template <typename K>
__host__ __device__ __forceinline__ K vox_flat_key(const int c[3], const VoxGeom& g) {
  return (static_cast<K>(c[2]) * g.grid[1] + c[1]) * g.grid[0] + c[0];
}
// flat key of a cell -> (z, y, x), the order the reference stores (:192)
__device__ __forceinline__ void vox_decode(uint64_t key, const VoxGeom& g, int& z, int& y, int& x) {
  x = static_cast<int>(key % g.grid[0]); key /= g.grid[0];
  y = static_cast<int>(key % g.grid[1]);
  z = static_cast<int>(key / g.grid[1]);
}
// Claims the table entry of `key` for point `index` (the smallest index of a key survives); returns the entry's slot.
__device__ __forceinline__ int vox_claim(uint64_t* __restrict__ table, uint32_t mask, uint64_t key, uint32_t index) {
  const uint64_t word = slot_pack(key, index);
  uint32_t h = hash_u64(key, mask);
  while (true) {
    unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(&table[h]),
                                       static_cast<unsigned long long>(kEmptySlot),
                                       static_cast<unsigned long long>(word));
    if (old == kEmptySlot) break;
    if (slot_key(old) == key) {
      atomicMin(reinterpret_cast<unsigned long long*>(&table[h]), static_cast<unsigned long long>(word));
      break;
    }
    h = (h + 1) & mask;
  }
  return static_cast<int>(h);
}

// ---- the two policies: which sample a row of the point buffer belongs to ------------------------------------------------------------
struct VoxOne {   // one cloud: no sample term, nothing read
  static constexpr int kStacked = 0;
  __device__ __forceinline__ uint64_t key_base(int64_t, const VoxGeom&) const { return 0; }
};
struct VoxStacked {   // B clouds back to back: off[b] <= rows of sample b < off[b + 1]
  static constexpr int kStacked = 1;
  const int* off;
  int batch;
  // sample of stacked row i: the b with off[b] <= i < off[b + 1] (empty samples have off[b] == off[b + 1] and own no row)
  __device__ __forceinline__ int sample_of(int i) const {
    int lo = 0, hi = batch;   // invariant: off[lo] <= i < off[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
  }
  __device__ __forceinline__ uint64_t volume(const VoxGeom& g) const { return static_cast<uint64_t>(g.grid[0]) * g.grid[1] * g.grid[2]; }
  __device__ __forceinline__ uint64_t key_base(int64_t i, const VoxGeom& g) const {
    return static_cast<uint64_t>(sample_of(static_cast<int>(i))) * volume(g);
  }
};

// scalars[0] = distinct voxels D, [1] = cut-off point index i*, [2] = kept points, [3] = M ([0], [1] and [3]: one cloud only)
template <class S>
__global__ void vox_insert(const float* __restrict__ pts, int64_t n, int ndim, VoxGeom g, S smp, uint64_t* __restrict__ table, uint32_t mask,
                           int* __restrict__ slot, int* __restrict__ scalars) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if constexpr (!S::kStacked) {
    if (i == 0) { scalars[1] = static_cast<int>(n); }   // no break unless vox_assign finds one
  }
  if (i >= n) return;
  int c[3];
  if (!vox_cell(pts + i * ndim, g, c)) { slot[i] = -1; return; }
  slot[i] = vox_claim(table, mask, smp.key_base(i, g) + vox_flat_key<uint64_t>(c, g), static_cast<uint32_t>(i));
}

// first[i] = 1 iff point i is the first of its voxel.  Stacked: first[] has n + 1 entries, the last one 0, so that the scan leaves the
// number of first points in rank[n].
template <class S>
__global__ void vox_mark_first(int64_t n, const uint64_t* __restrict__ table, const int* __restrict__ slot, int* __restrict__ first) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n + S::kStacked) return;
  int f = 0;
  if (!S::kStacked || i < n) {
    const int s = slot[i];
    f = (s >= 0 && slot_val(table[s]) == static_cast<uint32_t>(i)) ? 1 : 0;
  }
  first[i] = f;
}

// ---- step 3, one cloud ----------------------------------------------------------------------------------------------------------------
// rank[] holds the exclusive scan of the first-flags.
__global__ void vox_assign(int64_t n, const uint64_t* __restrict__ table, const int* __restrict__ slot,
                           const int* __restrict__ rank, VoxGeom g, int max_voxels, int* __restrict__ coors,
                           int* __restrict__ scalars) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = slot[i];
  if (s < 0) return;
  const uint64_t w = table[s];
  if (slot_val(w) != static_cast<uint32_t>(i)) return;  // not a first point
  const int v = rank[i];
  if (v == max_voxels) scalars[1] = static_cast<int>(i);  // unique writer: the reference's break point
  if (v >= max_voxels) return;
  int z, y, x;
  vox_decode(slot_key(w), g, z, y, x);
  coors[v * 3 + 0] = z; coors[v * 3 + 1] = y; coors[v * 3 + 2] = x;
}

__global__ void vox_words(int64_t n, const uint64_t* __restrict__ table, const int* __restrict__ slot,
                          const int* __restrict__ rank, const int* __restrict__ scalars,
                          uint64_t* __restrict__ words, int* __restrict__ count) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = slot[i];
  uint64_t w = ~0ull;
  if (s >= 0 && i < scalars[1]) {
    const int f = static_cast<int>(slot_val(table[s]));
    const int v = rank[f];
    atomicAdd(&count[v], 1);
    w = slot_pack(static_cast<uint64_t>(v), static_cast<uint32_t>(i));
  }
  words[i] = w;
}

__global__ void vox_finalize_scalars(int max_voxels, int* __restrict__ scalars, int* __restrict__ num_voxels) {
  const int d = scalars[0];
  const int m = d < max_voxels ? d : max_voxels;
  scalars[3] = m;
  *num_voxels = m;
}

// ---- step 3, stacked ------------------------------------------------------------------------------------------------------------------
constexpr int kOffChunk = 256;
struct VoxOffsets { int v[kOffChunk]; };

__global__ __launch_bounds__(kOffChunk) void vox_stack_offsets(VoxOffsets o, int first, int count, int* __restrict__ off) {
  const int t = threadIdx.x;
  int v = 0;
  // a compile-time index per lane keeps the argument block in scalar registers (a run-time index would copy it to scratch)
#pragma unroll
  for (int j = 0; j < kOffChunk; ++j) v = (j == t) ? o.v[j] : v;
  if (t < count) off[first + t] = v;
}

// One workgroup.  base[b] = first output row of sample b (base[batch] = rows produced), cut[b] = the stacked index at which sample b's
// scan breaks (off[b + 1] when it does not), voxel_cnt[b] = M_b.
__global__ __launch_bounds__(256) void vox_stack_bases(const int* __restrict__ off, int batch, const int* __restrict__ rank, int max_voxels,
                                                       int* __restrict__ base, int* __restrict__ cut, int* __restrict__ voxel_cnt) {
  __shared__ int lds_wave[4];
  int carry = 0;
  for (int c0 = 0; c0 < batch; c0 += 256) {
    const int b = c0 + static_cast<int>(threadIdx.x);
    int m = 0;
    if (b < batch) {
      const int lo = off[b], hi = off[b + 1];
      const int r0 = rank[lo], d = rank[hi] - r0;
      m = d < max_voxels ? d : max_voxels;
      int stop = hi;
      if (d > max_voxels) {
        // smallest i in [lo, hi) with rank[i + 1] > r0 + max_voxels: the first point of the sample's voxel number max_voxels
        int a = lo, z = hi - 1;   // rank[z + 1] = r0 + d > r0 + max_voxels holds at z = hi - 1
        while (a < z) {
          const int mid = (a + z) >> 1;
          if (rank[mid + 1] > r0 + max_voxels) z = mid; else a = mid + 1;
        }
        stop = a;
      }
      cut[b] = stop;
      voxel_cnt[b] = m;
    }
    int tot;
    const int ex = block_excl_scan_256(m, lds_wave, &tot);
    if (b < batch) base[b] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) base[batch] = carry;
}

// Assign and words in one pass: every kept point gets its (output row, stacked index) word and counts into its row; the first point
// of a voxel also writes the row's (b, z, y, x).
__global__ void vox_stack_words(int n, const uint64_t* __restrict__ table, const int* __restrict__ slot, const int* __restrict__ rank,
                                VoxStacked smp, const int* __restrict__ base, const int* __restrict__ cut, VoxGeom g,
                                uint64_t* __restrict__ words, int* __restrict__ count, int* __restrict__ coords) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = slot[i];
  uint64_t w = ~0ull;
  if (s >= 0) {
    const int b = smp.sample_of(static_cast<int>(i));
    if (i < cut[b]) {
      const uint64_t tw = table[s];
      const int f = static_cast<int>(slot_val(tw));
      const int row = base[b] + rank[f] - rank[smp.off[b]];   // f <= i < cut[b], so the rank inside the sample is below max_voxels
      atomicAdd(&count[row], 1);
      w = slot_pack(static_cast<uint64_t>(row), static_cast<uint32_t>(i));
      if (f == static_cast<int>(i)) {
        int z, y, x;
        vox_decode(slot_key(tw) - static_cast<uint64_t>(b) * smp.volume(g), g, z, y, x);
        int* q = coords + static_cast<int64_t>(row) * 4;
        q[0] = b; q[1] = z; q[2] = y; q[3] = x;
      }
    }
  }
  words[i] = w;
}

// ---- step 4 ---------------------------------------------------------------------------------------------------------------------------
// start[] = exclusive scan of count[]; scalars[2] = kept points.
__global__ void vox_fill(int64_t n, const float* __restrict__ pts, int ndim, const uint64_t* __restrict__ words,
                         const int* __restrict__ start, const int* __restrict__ scalars, int max_points,
                         float* __restrict__ voxels, int* __restrict__ num_per_voxel) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= n || p >= scalars[2]) return;
  const uint64_t w = words[p];
  const int v = static_cast<int>(slot_key(w));
  const int64_t i = slot_val(w);
  const int pos = static_cast<int>(p) - start[v];
  if (pos == 0) {
    const int cnt = start[v + 1] - start[v];
    num_per_voxel[v] = cnt < max_points ? cnt : max_points;
  }
  if (pos < max_points) {
    float* dst = voxels + (static_cast<int64_t>(v) * max_points + pos) * ndim;
    const float* src = pts + i * ndim;
    for (int j = 0; j < ndim; ++j) dst[j] = src[j];
  }
}

// MeanVFE straight from the sorted words: the sum over a row's first min(points, max_points) slots in slot order / max(that, 1) — the
// arithmetic of voxel_mean_collate (sparse_aux.hip), whose further slots are zero padding that leaves the fp32 sum as it is.
__global__ __launch_bounds__(256) void vox_stack_mean(int64_t total, const float* __restrict__ pts, int ndim, const uint64_t* __restrict__ words,
                                                      const int* __restrict__ start, const int* __restrict__ rows, int max_points,
                                                      float* __restrict__ feats) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= total) return;
  const int v = static_cast<int>(t / ndim), d = static_cast<int>(t % ndim);
  if (v >= *rows) return;
  const int p0 = start[v], cnt = start[v + 1] - p0;
  const int k = cnt < max_points ? cnt : max_points;
  float s = 0.f;
  for (int p = 0; p < k; ++p) s += pts[static_cast<int64_t>(slot_val(words[p0 + p])) * ndim + d];
  feats[t] = s / static_cast<float>(k < 1 ? 1 : k);
}

// ---- host side: one workspace, one front, one tail ------------------------------------------------------------------------------------
struct VoxWs {
  uint64_t* table; uint32_t cap;
  int* off; int* base; int* cut;   // stacked only
  int* slot; int* rank; int* count; int* scalars;
  uint64_t* words; uint64_t* tmp;
  char* aux; size_t aux_bytes;
};

// The workspace of n points and at most `rows` output rows; batch = 0: one cloud.  C is a Carver, or a Sizer for the size queries.
// rows: max_voxels for one cloud; stacked, an upper bound of the packed rows (the call's own sum of min(n_b, max_voxels), or
// min(n, B * max_voxels) for the query).
template <typename C>
static VoxWs vox_carve(C& c, int64_t n, int batch, int64_t rows) {
  const int64_t ranks = n + (batch ? 1 : 0);
  VoxWs w = {};
  w.cap = next_pow2(static_cast<uint64_t>(n > 512 ? n : 512) * 2);
  w.aux_bytes = radix_sort_ws_bytes(n);
  const size_t a2 = scan_ws_bytes(ranks > rows + 1 ? ranks : rows + 1);
  if (a2 > w.aux_bytes) w.aux_bytes = a2;
  w.table = c.template take<uint64_t>(w.cap);
  if (batch) {
    w.off = c.template take<int>(static_cast<size_t>(batch) + 1);
    w.base = c.template take<int>(static_cast<size_t>(batch) + 1);
    w.cut = c.template take<int>(static_cast<size_t>(batch));
  }
  w.slot = c.template take<int>(n);
  w.rank = c.template take<int>(ranks);
  w.count = c.template take<int>(rows + 2);
  w.scalars = c.template take<int>(8);
  w.words = c.template take<uint64_t>(n);
  w.tmp = c.template take<uint64_t>(n);
  w.aux = c.template take<char>(w.aux_bytes);
  return w;
}
static size_t vox_ws_bytes(int64_t n, int batch, int64_t rows) {
  Sizer s;
  vox_carve(s, n, batch, rows);
  return s.bytes();
}

// The limits both device entry points share, after their own size and pointer checks (batch = 0: one cloud).
static int vox_check_limits(const char* who, int64_t n, int batch, int max_voxels, const int grid[3]) {
  const char* per = batch ? "batch * " : "";
  const int b = batch ? batch : 1;
  FV2P_REQUIRE(grid[0] > 0 && grid[1] > 0 && grid[2] > 0, FV2P_EINVAL, "%s: empty grid", who);
  FV2P_REQUIRE(n <= kMaxRows, FV2P_ELIMIT, "%s: more than %lld points", who, (long long)kMaxRows);
  FV2P_REQUIRE(static_cast<int64_t>(grid[0]) * grid[1] * grid[2] <= kMaxKey / b, FV2P_ELIMIT, "%s: %sgrid volume exceeds 2^40", who, per);
  FV2P_REQUIRE(static_cast<int64_t>(b) * max_voxels <= kMaxRows, FV2P_ELIMIT, "%s: %smax_voxels too large", who, per);
  return 0;
}

// Carves the workspace and clears it together with the outputs the caller has listed in `fill` (one launch).
static int vox_open(const char* who, void* ws, size_t ws_bytes, int64_t n, int batch, int max_voxels, int64_t rows, FillJobs& fill, VoxWs* w,
                    hipStream_t stream) {
  const size_t need = batch ? fv2p_points_to_voxel_stack_ws_bytes(n, batch, max_voxels) : fv2p_points_to_voxel_ws_bytes(n, max_voxels);
  FV2P_REQUIRE(ws && ws_bytes >= need, FV2P_EWORKSPACE, "%s: workspace too small", who);
  Carver c(ws, ws_bytes);
  *w = vox_carve(c, n, batch, rows);
  fill.add(w->table, sizeof(uint64_t) * w->cap, 0xFFFFFFFFu);
  fill.add(w->count, sizeof(int) * static_cast<size_t>(rows + 2), 0u);
  if (!batch) fill.add(w->scalars, sizeof(int) * 8, 0u);
  return multi_fill(fill, stream);
}

// Steps 1 and 2: rank[] = exclusive scan of the first-flags (one cloud: their total in scalars[0]; stacked: in rank[n]).
template <class S>
static int vox_rank_firsts(const S& smp, const float* points, int64_t n, int ndim, const VoxGeom& g, const VoxWs& w, hipStream_t stream) {
  const int T = 256;
  const int64_t ranks = n + S::kStacked;
  hipLaunchKernelGGL(vox_insert<S>, dim3(static_cast<unsigned>(ceil_div(n, T))), dim3(T), 0, stream, points, n, ndim, g, smp, w.table, w.cap - 1,
                     w.slot, w.scalars);
  hipLaunchKernelGGL(vox_mark_first<S>, dim3(static_cast<unsigned>(ceil_div(ranks, T))), dim3(T), 0, stream, n, w.table, w.slot, w.rank);
  return exclusive_scan_i32(w.rank, w.rank, ranks, S::kStacked ? nullptr : w.scalars + 0, w.aux, w.aux_bytes, stream);
}

// Step 4: the words sorted by output row (rows < `rows`, so the all-ones word of a dropped point sorts behind every kept one), count[]
// turned into the rows' start offsets, then the padded (voxels, num_points) - unless voxels is null: the caller reads the sorted words itself.
static int vox_sort_fill(const float* points, int64_t n, int ndim, int64_t rows, int max_points, const VoxWs& w, float* voxels, int* num_points,
                         hipStream_t stream) {
  const int vb = bits_for(static_cast<uint64_t>(rows));
  int rc = radix_sort_u64(w.words, w.tmp, n, kValBits, kValBits + vb, w.aux, w.aux_bytes, stream);
  if (rc) return rc;
  rc = exclusive_scan_i32(w.count, w.count, rows + 1, w.scalars + 2, w.aux, w.aux_bytes, stream);
  if (rc || !voxels) return rc;
  hipLaunchKernelGGL(vox_fill, dim3(static_cast<unsigned>(ceil_div(n, 256))), dim3(256), 0, stream, n, points, ndim, w.words, w.count, w.scalars,
                     max_points, voxels, num_points);
  return 0;
}

static int64_t vox_stack_rows_bound(int64_t n, int batch, int max_voxels) {
  const int64_t bm = static_cast<int64_t>(batch) * max_voxels;
  return n < bm ? n : bm;
}

// Both stacked forms: mean -> MeanVFE features, else padded (voxels, num_points).
static int vox_stack_run(bool mean, const float* points, int64_t n, int ndim, int batch, const int* counts, const float voxel_size[3],
                         const float range_lo[3], const int grid[3], int max_points, int max_voxels, float* voxels, float* feats,
                         int* coords, int* num_points, int* voxel_cnt, void* ws, size_t ws_bytes, hipStream_t stream, const char* who) {
  FV2P_REQUIRE(n >= 0 && ndim >= 3 && max_points >= 1 && max_voxels >= 1 && batch >= 1, FV2P_EINVAL,
               "%s: bad sizes n=%lld ndim=%d batch=%d max_points=%d max_voxels=%d", who, (long long)n, ndim, batch, max_points, max_voxels);
  FV2P_REQUIRE(counts && voxel_cnt && (points || n == 0), FV2P_EINVAL, "%s: null pointer", who);
  if (int rc = vox_check_limits(who, n, batch, max_voxels, grid)) return rc;
  int64_t sum = 0, rows_cap = 0;
  for (int b = 0; b < batch; ++b) {
    FV2P_REQUIRE(counts[b] >= 0, FV2P_EINVAL, "%s: negative point count of sample %d", who, b);
    sum += counts[b];
    rows_cap += counts[b] < max_voxels ? counts[b] : max_voxels;
  }
  FV2P_REQUIRE(sum == n, FV2P_EINVAL, "%s: the counts sum to %lld, not to the %lld points", who, (long long)sum, (long long)n);
  FV2P_REQUIRE(rows_cap == 0 || (coords && (mean ? feats != nullptr : voxels && num_points)), FV2P_EINVAL, "%s: null output pointer", who);
  FillJobs fill;
  if (mean) fill.add(feats, sizeof(float) * static_cast<size_t>(rows_cap) * ndim, 0u);
  else {
    fill.add(voxels, sizeof(float) * static_cast<size_t>(rows_cap) * max_points * ndim, 0u);
    fill.add(num_points, sizeof(int) * static_cast<size_t>(rows_cap), 0u);
  }
  fill.add(coords, sizeof(int) * 4 * static_cast<size_t>(rows_cap), 0u);
  fill.add(voxel_cnt, sizeof(int) * static_cast<size_t>(batch), 0u);
  if (n == 0) return multi_fill(fill, stream);
  VoxWs w;
  if (int rc = vox_open(who, ws, ws_bytes, n, batch, max_voxels, rows_cap, fill, &w, stream)) return rc;
  const VoxGeom g = vox_geom(voxel_size, range_lo, grid);
  {
    VoxOffsets o;
    int64_t run = 0;   // off[k] = points before sample k, k = 0 .. batch
    for (int first = 0; first <= batch; first += kOffChunk) {
      const int cnt = batch + 1 - first < kOffChunk ? batch + 1 - first : kOffChunk;
      for (int t = 0; t < kOffChunk; ++t) {
        o.v[t] = static_cast<int>(run);
        if (t < cnt && first + t < batch) run += counts[first + t];
      }
      hipLaunchKernelGGL(vox_stack_offsets, dim3(1), dim3(kOffChunk), 0, stream, o, first, cnt, w.off);
    }
  }
  const VoxStacked smp = {w.off, batch};
  if (int rc = vox_rank_firsts(smp, points, n, ndim, g, w, stream)) return rc;
  hipLaunchKernelGGL(vox_stack_bases, dim3(1), dim3(256), 0, stream, w.off, batch, w.rank, max_voxels, w.base, w.cut, voxel_cnt);
  hipLaunchKernelGGL(vox_stack_words, dim3(static_cast<unsigned>(ceil_div(n, 256))), dim3(256), 0, stream, static_cast<int>(n), w.table, w.slot,
                     w.rank, smp, w.base, w.cut, g, w.words, w.count, coords);
  if (int rc = vox_sort_fill(points, n, ndim, rows_cap, max_points, w, mean ? nullptr : voxels, num_points, stream)) return rc;
  if (mean) {
    const int64_t total = rows_cap * ndim;
    hipLaunchKernelGGL(vox_stack_mean, dim3(static_cast<unsigned>(ceil_div(total, 256))), dim3(256), 0, stream, total, points, ndim,
                       w.words, w.count, w.base + batch, max_points, feats);
  }
  FV2P_LAUNCH_CHECK();
  return 0;
}

}  // namespace fv2p

using namespace fv2p;

extern "C" size_t fv2p_points_to_voxel_stack_ws_bytes(int64_t n_total, int batch, int max_voxels) {
  if (n_total < 1) n_total = 1;
  if (batch < 1) batch = 1;
  if (max_voxels < 1) max_voxels = 1;
  return vox_ws_bytes(n_total, batch, vox_stack_rows_bound(n_total, batch, max_voxels));
}

extern "C" int fv2p_points_to_voxel_stack(const float* points, int64_t n_total, int ndim, int batch, const int* counts,
                                          const float voxel_size[3], const float range_lo[3], const int grid[3], int max_points,
                                          int max_voxels, float* voxels, int* coords, int* num_points, int* voxel_cnt, void* ws,
                                          size_t ws_bytes, fv2p_stream_t stream) {
  return vox_stack_run(false, points, n_total, ndim, batch, counts, voxel_size, range_lo, grid, max_points, max_voxels, voxels, nullptr, coords,
                       num_points, voxel_cnt, ws, ws_bytes, static_cast<hipStream_t>(stream), "points_to_voxel_stack");
}

extern "C" int fv2p_points_to_voxel_stack_mean(const float* points, int64_t n_total, int ndim, int batch, const int* counts,
                                               const float voxel_size[3], const float range_lo[3], const int grid[3], int max_points,
                                               int max_voxels, float* features, int* coords, int* voxel_cnt, void* ws, size_t ws_bytes,
                                               fv2p_stream_t stream) {
  return vox_stack_run(true, points, n_total, ndim, batch, counts, voxel_size, range_lo, grid, max_points, max_voxels, nullptr, features, coords,
                       nullptr, voxel_cnt, ws, ws_bytes, static_cast<hipStream_t>(stream), "points_to_voxel_stack_mean");
}

extern "C" size_t fv2p_points_to_voxel_ws_bytes(int64_t n_points, int max_voxels) {
  if (n_points < 1) n_points = 1;
  if (max_voxels < 1) max_voxels = 1;
  return vox_ws_bytes(n_points, 0, max_voxels);
}

extern "C" int fv2p_points_to_voxel(const float* points, int64_t n, int ndim, const float voxel_size[3],
                                    const float range_lo[3], const int grid[3], int max_points, int max_voxels,
                                    float* voxels, int* coors, int* num_points_per_voxel, int* num_voxels,
                                    void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const char* who = "points_to_voxel";
  FV2P_REQUIRE(n >= 0 && ndim >= 3 && max_points >= 1 && max_voxels >= 1, FV2P_EINVAL,
               "%s: bad sizes n=%lld ndim=%d max_points=%d max_voxels=%d", who, (long long)n, ndim, max_points, max_voxels);
  FV2P_REQUIRE(voxels && coors && num_points_per_voxel && num_voxels && (points || n == 0), FV2P_EINVAL, "%s: null pointer", who);
  if (int rc = vox_check_limits(who, n, 0, max_voxels, grid)) return rc;
  FillJobs fill;
  fill.add(voxels, sizeof(float) * max_voxels * (size_t)max_points * ndim, 0u);
  fill.add(coors, sizeof(int) * 3 * (size_t)max_voxels, 0u);
  fill.add(num_points_per_voxel, sizeof(int) * (size_t)max_voxels, 0u);
  fill.add(num_voxels, sizeof(int), 0u);
  if (n == 0) return multi_fill(fill, stream);
  VoxWs w;
  if (int rc = vox_open(who, ws, ws_bytes, n, 0, max_voxels, max_voxels, fill, &w, stream)) return rc;
  const VoxGeom g = vox_geom(voxel_size, range_lo, grid);
  if (int rc = vox_rank_firsts(VoxOne{}, points, n, ndim, g, w, stream)) return rc;
  const dim3 gridN(static_cast<unsigned>(ceil_div(n, 256))), block(256);
  hipLaunchKernelGGL(vox_assign, gridN, block, 0, stream, n, w.table, w.slot, w.rank, g, max_voxels, coors, w.scalars);
  hipLaunchKernelGGL(vox_finalize_scalars, dim3(1), dim3(1), 0, stream, max_voxels, w.scalars, num_voxels);
  hipLaunchKernelGGL(vox_words, gridN, block, 0, stream, n, w.table, w.slot, w.rank, w.scalars, w.words, w.count);
  if (int rc = vox_sort_fill(points, n, ndim, max_voxels, max_points, w, voxels, num_points_per_voxel, stream)) return rc;
  FV2P_LAUNCH_CHECK();
  return 0;
}


// ---- host entry point: the reference's own call site of A1 ---------------------------------------------------------------------------
// VoxelGenerator.generate runs inside forked DataLoader worker processes on numpy arrays (data_processor.py:43-81 -> voxel_generator.py:
// 75-207), where HIP cannot be initialised.  Like fv2p_points_in_boxes_cpu and fv2p_boxes_iou_bev_cpu this is the reference's CPU
// entry point served by the library on the calling thread (host pointers, no HIP call): the same sequential first-come scan, with an
// open-addressing table over the <= max_voxels voxels in place of the reference's dense coor_to_voxelidx grid (360 MB filled per call at
// the KITTI grid, :114).  Device inputs never come here (the Python layer sends CUDA tensors to fv2p_points_to_voxel).
extern "C" int fv2p_points_to_voxel_host(const float* points, int64_t n, int ndim, const float voxel_size[3], const float range_lo[3],
                                         const int grid[3], int max_points, int max_voxels, float* voxels, int* coors,
                                         int* num_points_per_voxel, int* num_voxels) {
  FV2P_REQUIRE(n >= 0 && ndim >= 3 && max_points >= 1 && max_voxels >= 0, FV2P_EINVAL, "points_to_voxel_host: bad sizes");
  FV2P_REQUIRE(num_voxels && (n == 0 || points) && (max_voxels == 0 || (voxels && coors && num_points_per_voxel)), FV2P_EINVAL,
               "points_to_voxel_host: null pointer");
  FV2P_REQUIRE(grid[0] > 0 && grid[1] > 0 && grid[2] > 0, FV2P_EINVAL, "points_to_voxel_host: empty grid");
  std::memset(voxels, 0, sizeof(float) * static_cast<size_t>(max_voxels) * max_points * ndim);
  std::memset(num_points_per_voxel, 0, sizeof(int) * static_cast<size_t>(max_voxels));
  size_t cap = 16;
  while (cap < 2 * static_cast<size_t>(max_voxels) + 2) cap <<= 1;
  std::vector<long long> keys(cap, -1);
  std::vector<int> vals(cap, 0);
  const VoxGeom g = vox_geom(voxel_size, range_lo, grid);
  int count = 0;
  for (int64_t i = 0; i < n; ++i) {
    const float* p = points + i * ndim;
    int c[3];
    if (!vox_cell(p, g, c)) continue;
    const long long key = vox_flat_key<long long>(c, g);
    size_t h = static_cast<size_t>(static_cast<unsigned long long>(key) * 0x9E3779B97F4A7C15ull) & (cap - 1);
    while (keys[h] != -1 && keys[h] != key) h = (h + 1) & (cap - 1);
    int idx;
    if (keys[h] == key) idx = vals[h];
    else {
      if (count >= max_voxels) break;   // (:198-199) the whole scan stops at the first point that would open voxel max_voxels + 1
      idx = count++;
      keys[h] = key; vals[h] = idx;
      coors[3 * idx + 0] = c[2]; coors[3 * idx + 1] = c[1]; coors[3 * idx + 2] = c[0];   // stored (z, y, x) (:192)
    }
    const int k = num_points_per_voxel[idx];
    if (k < max_points) {   // (:204-206)
      std::memcpy(voxels + (static_cast<size_t>(idx) * max_points + k) * ndim, p, sizeof(float) * ndim);
      num_points_per_voxel[idx] = k + 1;
    }
  }
  *num_voxels = count;
  return 0;
}
