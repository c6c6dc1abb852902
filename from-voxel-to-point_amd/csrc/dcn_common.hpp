// What the fp32 kernels of dcn.hip and the 16-bit kernels of dcn_h.hip / dcn_bwd_h.hip share: the geometry, the bilinear corner set-up, the XCD-major
// tile order, the LDS-DMA of a weight piece and the rule that cuts a batch into chunks of whole samples.
#pragma once
#include "common.hpp"
#include <algorithm>

namespace fv2p {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// G: convolution groups - input channels [g*Cin/G, (g+1)*Cin/G) feed output channels [g*Cout/G, (g+1)*Cout/G) only
struct DcnGeom {
  int B, H, W, Cin, Cout, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, dg, G;
};

// Workgroup b of a launch runs on XCD b % 8, each XCD with an L2 of its own.  Handing out tiles in launch order gives every XCD every
// eighth tile: the eight L2s then all hold the same band of the map (a tile's bilinear samples reach into its neighbours' pixels) and
// each line is fetched from the fabric eight times - 815 MB of L2 fills for 83 MB of input at [4,128,200,176], rocprofv3 FETCH_SIZE.
// XCD-major order gives every XCD one contiguous eighth of the tiles instead.  (tile, sub): sub is the fast index (column block / share).
__device__ __forceinline__ void xcd_tile(int n_sub, long long& tile, int& sub) {
  const long long total = gridDim.x, b = blockIdx.x;
  const long long x = b & 7, slot = b >> 3;
  const long long lp = x * (total >> 3) + (x < (total & 7) ? x : (total & 7)) + slot;
  tile = lp / n_sub;
  sub = static_cast<int>(lp % n_sub);
}

// 64 lanes x 16 bytes from global memory straight into 1 KB of LDS, lane-linear
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst) {
  const unsigned dst = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(reinterpret_cast<uintptr_t>(lds_dst)));
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
}

struct Corner4 {
  unsigned o[4];
  float w[4];
  float m;
};

// EB: bytes of one element of x (4: fp32 maps, 2: float16 / bfloat16 maps); positions and weights are fp32 either way
template <int EB = 4>
__device__ __forceinline__ void make_corners(const DcnGeom& g, bool live, int b, float h_im, float w_im, float m, unsigned lane_bytes, Corner4& t) {
  const bool valid = live && (h_im > -1.f && w_im > -1.f && h_im < static_cast<float>(g.H) && w_im < static_cast<float>(g.W));
  const float hf = floorf(h_im), wf = floorf(w_im);
  const int h_low = static_cast<int>(hf), w_low = static_cast<int>(wf);
  const int h_high = h_low + 1, w_high = w_low + 1;
  const float lh = h_im - hf, lw = w_im - wf, hh = 1.f - lh, hw = 1.f - lw;
  const bool hl = valid && h_low >= 0, hhi = valid && h_high <= g.H - 1, wl = w_low >= 0, whi = w_high <= g.W - 1;
  t.w[0] = (hl && wl) ? hh * hw : 0.f;
  t.w[1] = (hl && whi) ? hh * lw : 0.f;
  t.w[2] = (hhi && wl) ? lh * hw : 0.f;
  t.w[3] = (hhi && whi) ? lh * lw : 0.f;
  t.m = valid ? m : 0.f;
  const int h0 = min(max(h_low, 0), g.H - 1), h1 = min(max(h_high, 0), g.H - 1);
  const int w0 = min(max(w_low, 0), g.W - 1), w1 = min(max(w_high, 0), g.W - 1);
  const unsigned row0 = static_cast<unsigned>((b * g.H + h0) * g.W), row1 = static_cast<unsigned>((b * g.H + h1) * g.W);
  const unsigned pitch = static_cast<unsigned>(g.Cin) * static_cast<unsigned>(EB);
  t.o[0] = (row0 + w0) * pitch + lane_bytes;
  t.o[1] = (row0 + w1) * pitch + lane_bytes;
  t.o[2] = (row1 + w0) * pitch + lane_bytes;
  t.o[3] = (row1 + w1) * pitch + lane_bytes;
}

struct CornerB {
  unsigned o[4];
  float w[4];
  float m, lh, lw;
  unsigned vb;   // bit q: corner q is inside the map (and the sample valid)
};

// the backward's corners: make_corners plus the fractions and the in-map bits that grad_offset / grad_mask need
template <int EB = 4>
__device__ __forceinline__ void make_corners_b(const DcnGeom& g, bool live, int b, float h_im, float w_im, float m, unsigned lane_bytes, CornerB& t) {
  const bool valid = live && (h_im > -1.f && w_im > -1.f && h_im < static_cast<float>(g.H) && w_im < static_cast<float>(g.W));
  const float hf = floorf(h_im), wf = floorf(w_im);
  const int h_low = static_cast<int>(hf), w_low = static_cast<int>(wf);
  const int h_high = h_low + 1, w_high = w_low + 1;
  const float lh = h_im - hf, lw = w_im - wf, hh = 1.f - lh, hw = 1.f - lw;
  const bool hl = valid && h_low >= 0, hhi = valid && h_high <= g.H - 1, wl = w_low >= 0, whi = w_high <= g.W - 1;
  t.w[0] = (hl && wl) ? hh * hw : 0.f;
  t.w[1] = (hl && whi) ? hh * lw : 0.f;
  t.w[2] = (hhi && wl) ? lh * hw : 0.f;
  t.w[3] = (hhi && whi) ? lh * lw : 0.f;
  t.vb = (hl && wl ? 1u : 0u) | (hl && whi ? 2u : 0u) | (hhi && wl ? 4u : 0u) | (hhi && whi ? 8u : 0u);
  t.m = valid ? m : 0.f;
  t.lh = lh; t.lw = lw;
  const int h0 = min(max(h_low, 0), g.H - 1), h1 = min(max(h_high, 0), g.H - 1);
  const int w0 = min(max(w_low, 0), g.W - 1), w1 = min(max(w_high, 0), g.W - 1);
  const unsigned row0 = static_cast<unsigned>((b * g.H + h0) * g.W), row1 = static_cast<unsigned>((b * g.H + h1) * g.W);
  const unsigned pitch = static_cast<unsigned>(g.Cin) * static_cast<unsigned>(EB);
  t.o[0] = (row0 + w0) * pitch + lane_bytes;
  t.o[1] = (row0 + w1) * pitch + lane_bytes;
  t.o[2] = (row1 + w0) * pitch + lane_bytes;
  t.o[3] = (row1 + w1) * pitch + lane_bytes;
}

// sample lists of the backward's gather (dcn.hip, pass 2): entry = {src = pixel * K + tap, lh, lw}
struct DcnEntries {
  unsigned* src;
  float* lh;
  float* lw;
};

struct SizerC : Sizer {
  template <typename T> T* take(size_t n) { Sizer::take<T>(n); return nullptr; }
};

static inline int dcn_cu_count() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cus = n;
    else cus = 256;
  }
  return cus;
}

// dcn.hip, for the 16-bit backward of dcn_bwd_h.hip: the cap on a chunk's column gradients (fv2p_dcn_set_colg_cap), the sample lists
// of one chunk from offsets in format `om` (0 fp32, FV2P_DT_F16, FV2P_DT_BF16), and the fixed-order sum of weight-gradient partials
long long dcn_colg_cap();
int dcn_sample_lists(const DcnGeom& gc, const void* offset, int om, int* cursor, DcnEntries entries, void* sws, hipStream_t stream);
void dcn_reduce_launch(const float* partial, int chunks, long long per_chunk, float* out, bool accumulate, hipStream_t stream);

// Samples per launch sequence: the kernels address x, the column gradients and the sample lists with 32-bit offsets, so a call is
// cut into chunks of whole samples that stay below those limits (the reference's im2col_step chunking, modulated_deform_conv_cuda.cu:
// 85-118, serves the same purpose) - and, for the backward, below `colg_cap` bytes of column gradients, which bounds the workspace
// whatever the batch.  Per-pixel arithmetic does not depend on the chunking; the weight gradient adds the chunks in ascending order.
// elem_bytes: bytes of one element of x and y (offsets and masks are counted as fp32, their widest form).  The column gradients are
// counted at 4 bytes an element whatever elem_bytes: the 16-bit backward (2-byte colg) therefore cuts a batch exactly where the fp32
// backward does - `colg_cap` bounds what the fp32 route WOULD hold, the 16-bit workspace is half of it - and one
// fv2p_dcn_set_colg_cap value means the same chunks on both routes.
static inline int dcn_chunk_samples(const DcnGeom& g, bool backward, long long colg_cap, int elem_bytes = 4) {
  const long long K = static_cast<long long>(g.kh) * g.kw;
  const long long x_bytes = static_cast<long long>(g.H) * g.W * g.Cin * elem_bytes;
  const long long pix = static_cast<long long>(g.Ho) * g.Wo;
  long long bs = g.B > 0 ? g.B : 1;
  bs = std::min(bs, ((1ll << 32) - 1) / std::max(x_bytes, 1ll));
  bs = std::min(bs, ((1ll << 32) - 1) / std::max(pix * std::max<long long>(static_cast<long long>(g.Cout) * elem_bytes, g.dg * 2 * K * 4), 1ll));   // y / dy, offset
  if (backward) {
    bs = std::min(bs, std::max(1ll, colg_cap / std::max(pix * K * g.Cin * 4, 1ll)));   // the cap is a preference: never below one sample
    bs = std::min(bs, ((1ll << 32) - 1) / std::max(pix * K * g.Cin * 4, 1ll));         // ... the 32-bit limit on its column gradients is hard
    bs = std::min(bs, ((1ll << 31) - 1) / std::max(pix * g.dg * K, 1ll));
  }
  return static_cast<int>(bs);   // 0: one sample alone is above a limit
}

}  // namespace fv2p
