// Centre head at test time: heat-map peak decode and detections for a whole batch.
//
// fv2p_center_peaks replaces CenterAFHeadTemplate.predhm_based_predicted_boxes_generation_ssd
// (pcdet/models/dense_heads/center_af_head_template.py:518-598; :600-667 without the max-pool) - center_utils._nms, the two
// torch.topk of center_utils._topk, six _transpose_and_gather_feat and box_utils.decode_rot_binres, about 25 tensor-op launches -
// with two launches:
//   center_heat_keys     every cell of every class map: heat = hm * (hm == max of its 3x3 neighbourhood) as an order-preserving
//                        32-bit key (descending float order = descending unsigned order; -0.0f and 0.0f share a key, as they
//                        compare equal in torch.topk)
//   center_select_decode one workgroup per sample: an LDS histogram of the keys' top 12 bits gives the bin of the k-th largest key.
//                        Short form (at most 4096 keys from that bin upwards, the usual case): they are collected and bitonic-sorted
//                        whole on (key descending, index ascending).  Long form (the k-th key lies in a crowded bin, e.g. it is the
//                        zero of the suppressed cells): two more histograms (10 + 10 bits) give the k-th key itself, the larger keys
//                        are collected in any order and the ties of the k-th key in index order, and the k survivors are sorted.
//                        Then gather and decode.
// Nothing is added in floating point and no workgroup depends on another: the result is a function of the maps alone.
//
// fv2p_detections_fgscore replaces the single-class-NMS branch of Detector3DTemplate.post_processing_withfgscores
// (pcdet/models/detectors/detector3d_template.py:392-415) and model_nms_utils.class_agnostic_nms_withfgscore
// (pcdet/models/model_utils/model_nms_utils.py:27-50): one ordering-and-gather launch, the greedy pass of fv2p_nms_batch
// (iou3d.hip), one output launch.
#include "common.hpp"
#include <math.h>

namespace fv2p {
namespace {

constexpr int kSelThreads = 1024;   // center_select_decode, det_order: one workgroup of 16 waves per sample
constexpr int kMaxPeaks = 512;
constexpr int kMaxSorted = 4096;    // center_select_decode: candidates it sorts whole instead of searching the k-th key bit by bit
constexpr int kMaxClasses = 16;
constexpr int kMaxBins = 32;
constexpr int kMaxCandidates = 4096;
constexpr uint32_t kZeroKey = 0x80000000u;

__device__ __forceinline__ uint32_t order_key(float v) {
  uint32_t u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;   // -0.0f ties with 0.0f
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// (key descending, index ascending) as one descending 64-bit order; never 0 for a real entry
__device__ __forceinline__ unsigned long long entry_of(uint32_t key, uint32_t idx) {
  return (static_cast<unsigned long long>(key) << 32) | static_cast<unsigned long long>(0xffffffffu - idx);
}
__device__ __forceinline__ uint32_t entry_index(unsigned long long e) { return 0xffffffffu - static_cast<uint32_t>(e & 0xffffffffull); }

// ---- launch 1: heat keys.  One thread per group of four cells of a row; VEC: rows are multiples of four floats and 16-byte aligned,
// the centre of each of the three rows is one 16-byte load and the four keys one 16-byte store.
template <int VEC>
__global__ __launch_bounds__(256) void center_heat_keys(const float* __restrict__ hm, int nc, int h, int w, int maxpool,
                                                        uint32_t* __restrict__ keys, int64_t key_stride) {
  const int gw = (w + 3) >> 2;
  const int64_t groups = static_cast<int64_t>(nc) * h * gw;
  const int64_t g = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (g >= groups) return;
  const int b = blockIdx.y;
  const int gx = static_cast<int>(g % gw);
  const int64_t row = g / gw;            // c * h + y
  const int y = static_cast<int>(row % h);
  const int x0 = gx * 4;
  const float* base = hm + (static_cast<int64_t>(b) * nc * h + row) * w;
  const float ninf = -INFINITY;
  float v[3][6];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int yy = y - 1 + r;
    const bool rok = yy >= 0 && yy < h && (maxpool || r == 1);
    const float* p = base + static_cast<int64_t>(r - 1) * w;
    if (VEC) {
      float4 c4 = make_float4(ninf, ninf, ninf, ninf);
      if (rok) c4 = *reinterpret_cast<const float4*>(p + x0);
      v[r][1] = c4.x; v[r][2] = c4.y; v[r][3] = c4.z; v[r][4] = c4.w;
      v[r][0] = (rok && x0 > 0) ? p[x0 - 1] : ninf;
      v[r][5] = (rok && x0 + 4 < w) ? p[x0 + 4] : ninf;
    } else {
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const int xx = x0 - 1 + j;
        v[r][j] = (rok && xx >= 0 && xx < w) ? p[xx] : ninf;
      }
    }
  }
  uint32_t out[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float c = v[1][j + 1];
    float heat = c;
    if (maxpool) {
      float m = c;
#pragma unroll
      for (int r = 0; r < 3; ++r) m = fmaxf(m, fmaxf(v[r][j], fmaxf(v[r][j + 1], v[r][j + 2])));
      heat = c * (c == m ? 1.0f : 0.0f);
    }
    out[j] = order_key(heat);
  }
  uint32_t* dst = keys + static_cast<int64_t>(b) * key_stride + row * w + x0;
  if (VEC) {
    *reinterpret_cast<uint4*>(dst) = make_uint4(out[0], out[1], out[2], out[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < w) dst[j] = out[j];
  }
}

// ---- helpers of the one-workgroup-per-sample kernels (blockDim.x == kSelThreads) ----
// exclusive prefix sum of one int per thread in thread order; *total = the sum, in every thread
__device__ __forceinline__ int block_excl_scan_1024(int v, int* s_wave /*[16]*/, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  if (lane == 63) s_wave[wv] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < kSelThreads / 64; ++i) {
    const int t = s_wave[i];
    if (i < wv) base += t;
    tot += t;
  }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

// the bin, counted from the top, in which the `want`-th largest entry lies, and its rank inside that bin (1-based): sel[0], sel[1].
// hist has NB bins, NB a multiple of kSelThreads; sum of hist >= want >= 1.  Ends with a barrier.
template <int NB>
__device__ __forceinline__ void find_bin(const int* hist, int want, int* s_wave, int* sel) {
  constexpr int PER = NB / kSelThreads;
  const int top = NB - 1 - static_cast<int>(threadIdx.x) * PER;
  int s = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) s += hist[top - j];
  int total;
  const int excl = block_excl_scan_1024(s, s_wave, &total);
  if (excl < want && want <= excl + s) {
    int acc = excl;
    for (int j = 0; j < PER; ++j) {
      const int c = hist[top - j];
      if (want <= acc + c) { sel[0] = top - j; sel[1] = want - acc; break; }
      acc += c;
    }
  }
  __syncthreads();
}

// in-place bitonic sort of s[0..p), p a power of two, DESCENDING
__device__ __forceinline__ void bitonic_desc(unsigned long long* s, int p) {
  for (int k = 2; k <= p; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < p; i += blockDim.x) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long a = s[i], c = s[l];
          const bool desc = (i & k) == 0;
          if (desc ? a < c : a > c) { s[i] = c; s[l] = a; }
        }
      }
      __syncthreads();
    }
}

struct PeakArgs {
  const float *hm, *offset, *height, *dim, *rot, *iouscore;
  const uint32_t* keys;
  int64_t key_stride;
  int nc, h, w, k, bins, p2;
  float stride, voxel_x, voxel_y, range_x0, range_y0, per, half_per;
  float *boxes, *cls, *score;
  long long* cell;
  int* cls_id;
};

// ---- launch 2: selection and decode, one workgroup per sample
__global__ __launch_bounds__(kSelThreads) void center_select_decode(PeakArgs a) {
  __shared__ int s_hist[4096];
  __shared__ unsigned long long s_ent[kMaxSorted];
  __shared__ int s_wave[kSelThreads / 64];
  __shared__ int s_sel[2];
  __shared__ int s_cnt;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int hw = a.h * a.w, n = a.nc * hw;
  const uint32_t* keys = a.keys + static_cast<int64_t>(b) * a.key_stride;
  const uint4* keys4 = reinterpret_cast<const uint4*>(keys);
  const int n4 = static_cast<int>(a.key_stride >> 2);   // key_stride: n rounded up to a multiple of 4, the pad is never used
  constexpr int UN = 4;                                  // 16-byte loads in flight per thread
  constexpr int STEP = kSelThreads * UN;

  // three histogram passes over the sample's keys: bits [20,32), [10,20), [0,10) of the k-th largest key
  uint32_t prefix = 0;
  int want = a.k;
  bool sorted = false;                  // uniform: s_ent already holds the result
  for (int pass = 0; pass < 3; ++pass) {
    for (int i = tid; i < 4096; i += kSelThreads) s_hist[i] = 0;
    __syncthreads();
    // A max-pooled heat map is zero in eight cells of nine: a thread counts its zeros in a register and adds them once, so that
    // the lanes do not queue on one LDS address.  The zero key takes part in a pass when it shares the prefix found so far.
    const int shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0);
    const bool zero_in = pass == 0 || (kZeroKey >> (shift + 10)) == prefix;
    const int zero_bin = static_cast<int>((kZeroKey >> shift) & (pass == 0 ? 4095u : 1023u));
    int zeros = 0;
    for (int base = 0; base < n4; base += STEP) {
      uint4 q[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int i4 = base + u * kSelThreads + tid;
        q[u] = i4 < n4 ? keys4[i4] : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int i4 = base + u * kSelThreads + tid;
        const uint32_t kk[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool in = i4 < n4 && i4 * 4 + j < n;
          const uint32_t key = kk[j];
          if (!in) continue;
          if (key == kZeroKey) zeros += 1;
          else if (pass == 0) atomicAdd(&s_hist[key >> 20], 1);
          else if ((key >> (shift + 10)) == prefix) atomicAdd(&s_hist[(key >> shift) & 1023u], 1);
        }
      }
    }
    if (zero_in && zeros) atomicAdd(&s_hist[zero_bin], zeros);
    __syncthreads();
    if (pass == 0) find_bin<4096>(s_hist, want, s_wave, s_sel);
    else find_bin<1024>(s_hist, want, s_wave, s_sel);
    prefix = pass == 0 ? static_cast<uint32_t>(s_sel[0]) : ((prefix << 10) | static_cast<uint32_t>(s_sel[0]));
    want = s_sel[1];
    if (pass == 0) {
      // Short form: the keys from the k-th key's bin upwards are few (the usual case: k peaks stand out of a map of zeros).  They
      // are collected in one more pass and sorted whole - the order (key descending, index ascending) is the selection rule itself.
      // The streaming passes are what this kernel's time is made of (one CU's fetch rate): two of them instead of four.
      const int cand = (a.k - want) + s_hist[prefix];   // uniform: the k-th key's bin and every bin above it
      if (cand <= kMaxSorted) {
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        for (int base = 0; base < n4; base += STEP) {
          uint4 q[UN];
#pragma unroll
          for (int u = 0; u < UN; ++u) {
            const int i4 = base + u * kSelThreads + tid;
            q[u] = i4 < n4 ? keys4[i4] : make_uint4(0, 0, 0, 0);
          }
#pragma unroll
          for (int u = 0; u < UN; ++u) {
            const int i4 = base + u * kSelThreads + tid;
            const uint32_t kk[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (i4 < n4 && i4 * 4 + j < n && (kk[j] >> 20) >= prefix) {
                const int slot = atomicAdd(&s_cnt, 1);
                if (slot < kMaxSorted) s_ent[slot] = entry_of(kk[j], static_cast<uint32_t>(i4 * 4 + j));
              }
          }
        }
        int p = 1;
        while (p < cand) p <<= 1;
        for (int i = cand + tid; i < p; i += kSelThreads) s_ent[i] = 0ull;   // the pad of the sort orders last
        __syncthreads();
        bitonic_desc(s_ent, p);
        sorted = true;
        break;
      }
    }
    __syncthreads();
  }
  if (!sorted) {
    const uint32_t kth = prefix;          // the k-th largest key
    const int need = want;                // ties of it to take, in index order (>= 1)
    const int larger = a.k - need;        // keys above it

    // collection pass
    if (tid == 0) s_cnt = 0;
    for (int i = tid; i < a.p2; i += kSelThreads) s_ent[i] = 0ull;   // the pad of the sort orders last
    __syncthreads();
    int taken = 0;                        // uniform
    for (int base = 0; base < n4; base += STEP) {
      uint4 q[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int i4 = base + u * kSelThreads + tid;
        q[u] = i4 < n4 ? keys4[i4] : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int i4 = base + u * kSelThreads + tid;
        const uint32_t kk[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
        int ties = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool in = i4 < n4 && i4 * 4 + j < n;
          if (in && kk[j] > kth) {
            const int slot = atomicAdd(&s_cnt, 1);
            if (slot < larger) s_ent[slot] = entry_of(kk[j], static_cast<uint32_t>(i4 * 4 + j));
          }
          ties += (in && kk[j] == kth) ? 1 : 0;
        }
        if (taken < need) {               // uniform: the barriers below are reached by every thread or by none
          if (__syncthreads_or(ties)) {
            int total;
            int rank = taken + block_excl_scan_1024(ties, s_wave, &total);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const bool in = i4 < n4 && i4 * 4 + j < n;
              if (in && kk[j] == kth) {
                if (rank < need) s_ent[larger + rank] = entry_of(kth, static_cast<uint32_t>(i4 * 4 + j));
                ++rank;
              }
            }
            taken += total;
          }
        }
      }
    }
    __syncthreads();
    bitonic_desc(s_ent, a.p2);
  }

  // gather and decode
  if (tid < a.k) {
    const uint32_t idx = entry_index(s_ent[tid]);
    const int c = static_cast<int>(idx / static_cast<uint32_t>(hw)), cell = static_cast<int>(idx % static_cast<uint32_t>(hw));
    const int y = cell / a.w, x = cell % a.w;
    const int64_t o = static_cast<int64_t>(b) * a.k + tid;
    const int64_t bhw = static_cast<int64_t>(b) * hw;
    const float off_x = a.offset[bhw * 2 + cell], off_y = a.offset[bhw * 2 + hw + cell];
    float* box = a.boxes + o * 7;
    // every product and sum rounded on its own, in the order of the tensor ops
    box[0] = __fadd_rn(__fmul_rn(__fmul_rn(__fadd_rn(static_cast<float>(x), off_x), a.stride), a.voxel_x), a.range_x0);
    box[1] = __fadd_rn(__fmul_rn(__fmul_rn(__fadd_rn(static_cast<float>(y), off_y), a.stride), a.voxel_y), a.range_y0);
    box[2] = a.height[bhw + cell];
#pragma unroll
    for (int j = 0; j < 3; ++j) box[3 + j] = a.dim[bhw * 3 + static_cast<int64_t>(j) * hw + cell];
    const float* r = a.rot + bhw * 2 * a.bins + cell;
    int which = 0;
    float best = r[0];
    for (int i = 1; i < a.bins; ++i) {
      const float v = r[static_cast<int64_t>(i) * hw];
      if (v > best) { best = v; which = i; }
    }
    const float res = __fmul_rn(r[static_cast<int64_t>(a.bins + which) * hw], a.half_per);
    const float two_pi = 6.283185307179586f, pi = 3.141592653589793f;
    float ry = fmodf(__fadd_rn(__fmul_rn(static_cast<float>(which), a.per), res), two_pi);   // torch.remainder: fmod, then the sign of the divisor
    if (ry != 0.0f && ry < 0.0f) ry = __fadd_rn(ry, two_pi);
    if (ry > pi) ry = __fsub_rn(ry, two_pi);
    box[6] = ry;
    for (int c2 = 0; c2 < a.nc; ++c2) {
      const uint32_t kk = keys[static_cast<int64_t>(c2) * hw + cell];
      const float src = a.hm[(static_cast<int64_t>(b) * a.nc + c2) * hw + cell];
      a.cls[o * a.nc + c2] = kk == kZeroKey ? __fmul_rn(src, 0.0f) : key_value(kk);   // the zero of a suppressed cell keeps the logit's sign
    }
    a.score[o] = a.iouscore[bhw + cell];
    a.cell[o] = cell;
    a.cls_id[o] = c;
  }
}

// ---- detections ----
// foreground score and label of one candidate: the first maximal class, of the sigmoid when the scores are logits
__device__ __forceinline__ float fg_score(const float* __restrict__ row, int nc, int normalized, int* label) {
  float best = 0.f;
  int arg = 0;
  for (int c = 0; c < nc; ++c) {
    float v = row[c];
    if (!normalized) v = 1.0f / (1.0f + expf(-v));
    if (c == 0 || v > best) { best = v; arg = c; }
  }
  *label = arg + 1;
  return best;
}

// gate, order by (loc score descending, index ascending), cut at m = min(n, pre_max), gather the boxes for the greedy pass.
// A slot without a candidate holds a zero-sized box far outside any scene, each at its own place: its IoU with every box is 0.
__global__ __launch_bounds__(kSelThreads) void det_order(const float* __restrict__ boxes, const float* __restrict__ cls,
                                                         const float* __restrict__ loc, int n, int nc, int normalized, float score_thresh,
                                                         int m, int p2, float* __restrict__ nms_boxes, int* __restrict__ order,
                                                         int* __restrict__ nvalid) {
  __shared__ unsigned long long s_ent[kMaxCandidates];
  __shared__ int s_cnt;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (int i = tid; i < p2; i += kSelThreads) {
    unsigned long long e = 0ull;
    if (i < n) {
      int label;
      const float fg = fg_score(cls + (static_cast<int64_t>(b) * n + i) * nc, nc, normalized, &label);
      if (fg >= score_thresh) {
        e = entry_of(order_key(loc[static_cast<int64_t>(b) * n + i]), static_cast<uint32_t>(i));
        atomicAdd(&s_cnt, 1);
      }
    }
    s_ent[i] = e;
  }
  __syncthreads();
  bitonic_desc(s_ent, p2);
  if (tid == 0) nvalid[b] = s_cnt < m ? s_cnt : m;
  for (int j = tid; j < m; j += kSelThreads) {
    const unsigned long long e = s_ent[j];
    float* dst = nms_boxes + (static_cast<int64_t>(b) * m + j) * 7;
    if (e) {
      const int i = static_cast<int>(entry_index(e));
      const float* src = boxes + (static_cast<int64_t>(b) * n + i) * 7;
#pragma unroll
      for (int t = 0; t < 7; ++t) dst[t] = src[t];
      order[static_cast<int64_t>(b) * m + j] = i;
    } else {
      dst[0] = 1.0e6f + 64.0f * static_cast<float>(j);
#pragma unroll
      for (int t = 1; t < 7; ++t) dst[t] = 0.f;
      order[static_cast<int64_t>(b) * m + j] = -1;
    }
  }
}

// survivors of the greedy pass come in ascending order: the real candidates first, then the empty slots
__global__ __launch_bounds__(256) void det_emit(const float* __restrict__ boxes, const float* __restrict__ cls, const float* __restrict__ loc,
                                                int n, int nc, int normalized, int m, int post_max, const long long* __restrict__ keep,
                                                const int* __restrict__ num_keep, const int* __restrict__ order, const int* __restrict__ nvalid,
                                                float* __restrict__ out_boxes, float* __restrict__ out_scores, int* __restrict__ out_labels,
                                                long long* __restrict__ out_index, int* __restrict__ count) {
  __shared__ int s_cnt;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  const int nk = num_keep[b] < post_max ? num_keep[b] : post_max, nv = nvalid[b];
  int mine = 0;
  for (int j = tid; j < post_max; j += 256) {
    const int64_t o = static_cast<int64_t>(b) * post_max + j;
    int slot = -1;
    if (j < nk) {
      const long long s = keep[static_cast<int64_t>(b) * m + j];
      if (s >= 0 && s < nv) slot = static_cast<int>(s);
    }
    if (slot >= 0) {
      const int i = order[static_cast<int64_t>(b) * m + slot];
      const float* src = boxes + (static_cast<int64_t>(b) * n + i) * 7;
#pragma unroll
      for (int t = 0; t < 7; ++t) out_boxes[o * 7 + t] = src[t];
      int label;
      fg_score(cls + (static_cast<int64_t>(b) * n + i) * nc, nc, normalized, &label);
      out_scores[o] = loc[static_cast<int64_t>(b) * n + i];
      out_labels[o] = label;
      out_index[o] = i;
      ++mine;
    } else {
#pragma unroll
      for (int t = 0; t < 7; ++t) out_boxes[o * 7 + t] = 0.f;
      out_scores[o] = 0.f;
      out_labels[o] = 0;
      out_index[o] = -1;
    }
  }
  if (mine) atomicAdd(&s_cnt, mine);
  __syncthreads();
  if (tid == 0) count[b] = s_cnt;
}

struct DetWs {
  float* nms_boxes;
  int* order;
  int* nvalid;
  long long* keep;
  int* num_keep;
  void* nms_ws;
  size_t nms_bytes;
};
template <typename C>
DetWs det_layout(C& c, int batch, int m, int post_max) {
  DetWs d;
  const size_t bm = static_cast<size_t>(batch) * m;
  d.nms_boxes = c.template take<float>(bm * 7);
  d.order = c.template take<int>(bm);
  d.nvalid = c.template take<int>(static_cast<size_t>(batch));
  d.keep = c.template take<long long>(bm);
  d.num_keep = c.template take<int>(static_cast<size_t>(batch));
  d.nms_bytes = fv2p_nms_batch_ws_bytes(batch, m, post_max);
  d.nms_ws = c.template take<char>(d.nms_bytes);
  return d;
}

int64_t peak_key_stride(int nc, int h, int w) { return (static_cast<int64_t>(nc) * h * w + 3) / 4 * 4; }

}  // namespace
}  // namespace fv2p
using namespace fv2p;

extern "C" size_t fv2p_center_peaks_ws_bytes(int batch, int nc, int h, int w) {
  if (batch <= 0 || nc <= 0 || h <= 0 || w <= 0) return 0;
  Sizer s;
  s.take<uint32_t>(static_cast<size_t>(batch) * static_cast<size_t>(peak_key_stride(nc, h, w)));
  return s.bytes();
}

extern "C" int fv2p_center_peaks(const float* hm, const float* offset, const float* height, const float* dim, const float* rot,
                                 const float* iouscore, int batch, int nc, int h, int w, int k, int maxpool, int bins, int stride, float voxel_x,
                                 float voxel_y, float range_x0, float range_y0, float* boxes, float* cls, float* score, int64_t* cell, int* cls_id,
                                 void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FV2P_REQUIRE(batch >= 1 && nc >= 1 && h >= 1 && w >= 1, FV2P_EINVAL, "center_peaks: batch %d, nc %d, h %d, w %d must be positive", batch, nc, h, w);
  FV2P_REQUIRE(nc <= kMaxClasses, FV2P_EINVAL, "center_peaks: nc %d above %d", nc, kMaxClasses);
  FV2P_REQUIRE(bins >= 1 && bins <= kMaxBins, FV2P_EINVAL, "center_peaks: bins %d outside 1 .. %d", bins, kMaxBins);
  FV2P_REQUIRE(k >= 1 && k <= kMaxPeaks && k <= static_cast<int64_t>(h) * w, FV2P_EINVAL, "center_peaks: k %d outside 1 .. min(%d, h * w)", k, kMaxPeaks);
  FV2P_REQUIRE((maxpool == 0 || maxpool == 1) && stride >= 1, FV2P_EINVAL, "center_peaks: maxpool %d is neither 0 nor 1, or stride %d < 1", maxpool, stride);
  FV2P_REQUIRE(hm && offset && height && dim && rot && iouscore && boxes && cls && score && cell && cls_id, FV2P_EINVAL, "center_peaks: null pointer");
  FV2P_REQUIRE(static_cast<int64_t>(nc) * h * w < (1ll << 31) - 4096 && batch <= 65535, FV2P_ELIMIT, "center_peaks: nc * h * w from 2^31 - 4096 or batch above 65535");
  FV2P_REQUIRE(ws && ws_bytes >= fv2p_center_peaks_ws_bytes(batch, nc, h, w), FV2P_EWORKSPACE, "center_peaks: workspace too small");
  Carver c(ws, ws_bytes);
  const int64_t key_stride = peak_key_stride(nc, h, w);
  uint32_t* keys = c.take<uint32_t>(static_cast<size_t>(batch) * static_cast<size_t>(key_stride));
  const int64_t groups = static_cast<int64_t>(nc) * h * ((w + 3) / 4);
  const dim3 grid(static_cast<unsigned>(ceil_div(groups, 256)), batch);
  // 16-byte accesses: whole rows of four-float groups from an aligned base (then every row and every key group is aligned)
  const bool vec = w % 4 == 0 && reinterpret_cast<uintptr_t>(hm) % 16 == 0;
  if (vec) hipLaunchKernelGGL(center_heat_keys<1>, grid, dim3(256), 0, stream, hm, nc, h, w, maxpool, keys, key_stride);
  else hipLaunchKernelGGL(center_heat_keys<0>, grid, dim3(256), 0, stream, hm, nc, h, w, maxpool, keys, key_stride);
  PeakArgs a;
  a.hm = hm; a.offset = offset; a.height = height; a.dim = dim; a.rot = rot; a.iouscore = iouscore;
  a.keys = keys; a.key_stride = key_stride;
  a.nc = nc; a.h = h; a.w = w; a.k = k; a.bins = bins; a.p2 = static_cast<int>(next_pow2(static_cast<uint64_t>(k)));
  a.stride = static_cast<float>(stride); a.voxel_x = voxel_x; a.voxel_y = voxel_y; a.range_x0 = range_x0; a.range_y0 = range_y0;
  const double per = 2.0 * M_PI / bins;     // decode_rot_binres: the angle of a bin in double, then one rounding
  a.per = static_cast<float>(per); a.half_per = static_cast<float>(per / 2.0);
  a.boxes = boxes; a.cls = cls; a.score = score; a.cell = reinterpret_cast<long long*>(cell); a.cls_id = cls_id;
  hipLaunchKernelGGL(center_select_decode, dim3(batch), dim3(kSelThreads), 0, stream, a);
  FV2P_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t fv2p_detections_fgscore_ws_bytes(int batch, int n, int pre_max, int post_max) {
  if (batch <= 0 || n <= 0 || pre_max <= 0 || post_max <= 0) return 0;
  Sizer s;
  det_layout(s, batch, n < pre_max ? n : pre_max, post_max);
  return s.bytes();
}

extern "C" int fv2p_detections_fgscore(const float* boxes, const float* cls, const float* loc_score, int batch, int n, int nc, int normalized,
                                       float score_thresh, float nms_thresh, int pre_max, int post_max, float* out_boxes, float* out_scores,
                                       int* out_labels, int64_t* out_index, int* count, void* ws, size_t ws_bytes, fv2p_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  FV2P_REQUIRE(batch >= 1 && nc >= 1 && n >= 1 && n <= kMaxCandidates, FV2P_EINVAL, "detections_fgscore: batch %d, nc %d or n %d outside 1 .. %d", batch, nc, n, kMaxCandidates);
  FV2P_REQUIRE(pre_max >= 1 && post_max >= 1 && post_max <= n, FV2P_EINVAL, "detections_fgscore: pre_max %d < 1 or post_max %d outside 1 .. n", pre_max, post_max);
  FV2P_REQUIRE(normalized == 0 || normalized == 1, FV2P_EINVAL, "detections_fgscore: normalized %d is neither 0 nor 1", normalized);
  FV2P_REQUIRE(boxes && cls && loc_score && out_boxes && out_scores && out_labels && out_index && count, FV2P_EINVAL, "detections_fgscore: null pointer");
  FV2P_REQUIRE(batch <= 65535, FV2P_ELIMIT, "detections_fgscore: batch above 65535");
  FV2P_REQUIRE(ws && ws_bytes >= fv2p_detections_fgscore_ws_bytes(batch, n, pre_max, post_max), FV2P_EWORKSPACE, "detections_fgscore: workspace too small");
  const int m = n < pre_max ? n : pre_max;
  Carver c(ws, ws_bytes);
  const DetWs d = det_layout(c, batch, m, post_max);
  hipLaunchKernelGGL(det_order, dim3(batch), dim3(kSelThreads), 0, stream, boxes, cls, loc_score, n, nc, normalized, score_thresh, m,
                     static_cast<int>(next_pow2(static_cast<uint64_t>(n))), d.nms_boxes, d.order, d.nvalid);
  FV2P_LAUNCH_CHECK();
  const int rc = fv2p_nms_batch(d.nms_boxes, batch, m, nms_thresh, 0, post_max, reinterpret_cast<int64_t*>(d.keep), m, d.num_keep, d.nms_ws,
                                d.nms_bytes, stream_);
  if (rc) return rc;
  hipLaunchKernelGGL(det_emit, dim3(batch), dim3(256), 0, stream, boxes, cls, loc_score, n, nc, normalized, m, post_max, d.keep, d.num_keep,
                     d.order, d.nvalid, out_boxes, out_scores, out_labels, reinterpret_cast<long long*>(out_index), count);
  FV2P_LAUNCH_CHECK();
  return 0;
}
