// A13 on float16 / bfloat16 maps: the forward of the modulated deformable convolution on v_mfma_f32_16x16x32_{f16,bf16}.
//
// The implicit GEMM of dcn_fwd_k (dcn.hip) in 16-bit storage: x NHWC [B,H,W,Cin], wt_oc [K][Cout][Cin] and y [B*Ho*Wo][Cout] hold
// 16-bit elements and no fp32 copy of any of them exists.  The product is formed transposed as there: A = weights (rows = output
// channels, from LDS), B = modulated bilinear samples (columns = pixels, in the registers of the lane that gathered them).  The operand
// layout of the 16x16x32 instruction - A[l & 15][8 (l >> 4) + j], B[8 (l >> 4) + j][l & 15], C/D col = l & 15, row = 4 (l >> 4) + reg -
// fits the fp32 kernel's scheme: lane (n, gq) gathers the 8 consecutive channels c0 + 8 gq .. + 7 of pixel n at each of the four
// bilinear corners (one 16-byte load each), and a weight fragment of 16 output channels x 32 input channels is 1 KB of 16-byte lane
// pieces, each contiguous in wt_oc, fetched by the LDS-DMA in lane-linear order and double-buffered.  A step is (tap, 32 input
// channels); the steps run in the fixed order (tap, deformable group, chunk).
//
// Arithmetic of one sample element: the four corner values widened, w0 v0 + w1 v1 + w2 v2 + w3 v3 in fp32 as the explicit fmaf chain
// of dcn_fwd_k's `combine`, times the mask, rounded to nearest even ONCE into the B operand.  Accumulators are fp32; the bias is
// added in fp32; one rounding at the store.  No atomics: two runs give the same bits.  Offsets and masks are fp32 or 16-bit
// (om_dtype) and are widened on load, positions are always formed in fp32.
//
// A deformable group whose width is 16 mod 32 ends in a 16-channel chunk: a 32-step whose upper half (lanes gq >= 2) is ZERO IN BOTH
// OPERANDS.  Those lanes fetch what the lanes gq - 2 fetch (addresses inside the group, so nothing outside x or wt_oc is ever read)
// and replace it with zeros before the MFMA: 0 x 0, never 0 x (whatever lies behind the group).
#include "common.hpp"
#include "dcn_common.hpp"
#include "dt16.hpp"
#include <algorithm>

namespace fv2p {

using f16x8 = _Float16 __attribute__((ext_vector_type(8)));
using bf16x8 = __bf16 __attribute__((ext_vector_type(8)));

struct DcnH16 : H16 {
  static __device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};
struct DcnB16 : B16 {
  static __device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};

// offset / mask element i: fp32 (om16 == 0) or the call's 16-bit format
template <class T>
__device__ __forceinline__ float om_load(const void* p, long long i, int om16) {
  return om16 ? T::widen(static_cast<const u16*>(p)[i]) : static_cast<const float*>(p)[i];
}

// Block = 4 waves, wave = 16 pixels x NB*16 output channels; n_sub column blocks of NB*16 per pixel tile.  Deformable group dgi holds
// the chunks j = 0 .. cps - 1 of 32 channels at dgi * cpg + 32 j; with `tail` the last one is 16 wide.
template <class T, int NB>
__global__ __launch_bounds__(256, 2) void dcn_fwd_h_k(DcnGeom g, const u16* __restrict__ x, const u16* __restrict__ wt_oc,
                                                       const float* __restrict__ bias, const void* __restrict__ offset,
                                                       const void* __restrict__ mask, int om16, u16* __restrict__ y, int n_sub) {
  extern __shared__ __attribute__((aligned(16))) uint4 lds_h[];   // 2 x NB pieces of 64 x 16 bytes
  constexpr int FRAG = NB * 64;                                   // in uint4
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n = lane & 15, gq = lane >> 4;
  const long long npix = static_cast<long long>(g.B) * g.Ho * g.Wo;
  const int plane = g.Ho * g.Wo;
  const int K = g.kh * g.kw, cpg = g.Cin / g.dg, cps = (cpg + 31) / 32;
  const bool tail = (cpg & 31) != 0;   // cpg = 16 mod 32
  long long tile;
  int cb;
  xcd_tile(n_sub, tile, cb);
  const int col0 = cb * (NB * 16);
  const int steps = K * g.dg * cps;
  const long long pix = tile * 64 + wave * 16 + n;
  const bool live = pix < npix;
  const long long pp = live ? pix : 0;
  const int pb = static_cast<int>(pp / plane), ppos = static_cast<int>(pp % plane), pho = ppos / g.Wo, pwo = ppos % g.Wo;
  // lanes of the upper half of a 16-channel step: addresses of the lanes gq - 2, operands zeroed
  const int gqh = gq & 1;
  const bool upper = gq >= 2;
  // weight rows this lane feeds to the LDS-DMA: piece nb, lane (n, gq) <- wt_oc[k][col0 + nb*16 + n][c0 + 8 gq ..] (rows clamped to Cout - 1)
  constexpr int NDMA = (NB + 3) / 4;
  const u16* wrow[NDMA];
#pragma unroll
  for (int i = 0; i < NDMA; ++i) {
    const int nb = wave + 4 * i;
    const int co = min(col0 + nb * 16 + n, g.Cout - 1);
    wrow[i] = wt_oc + static_cast<long long>(co) * g.Cin;
  }
  auto dma = [&](int k, int c0, bool half, uint4* buf) {
    const long long at = static_cast<long long>(k) * g.Cout * g.Cin + c0 + 8 * (half ? gqh : gq);
#pragma unroll
    for (int i = 0; i < NDMA; ++i) {
      const int nb = wave + 4 * i;
      if (nb < NB) glds16(wrow[i] + at, buf + nb * 64);
    }
  };
  Corner4 t;
  float roh, row_, rom;   // raw offsets / mask of the NEXT (tap, group) segment
  auto load_offsets = [&](int k, int dgi) {
    const long long ob = (static_cast<long long>(pb) * g.dg + dgi) * 2 * K * plane + ppos;
    roh = om_load<T>(offset, ob + static_cast<long long>(2 * k) * plane, om16);
    row_ = om_load<T>(offset, ob + static_cast<long long>(2 * k + 1) * plane, om16);
    rom = om_load<T>(mask, ((static_cast<long long>(pb) * g.dg + dgi) * K + k) * plane + ppos, om16);
  };
  auto set_taps = [&](int k) {
    const int i = k / g.kw, j = k % g.kw;
    const float h_im = static_cast<float>(pho * g.sh - g.ph + i * g.dh) + roh;
    const float w_im = static_cast<float>(pwo * g.sw - g.pw + j * g.dw) + row_;
    make_corners<2>(g, live, pb, h_im, w_im, rom, 0u, t);
  };
  uint4 raw[4];
  auto gather = [&](int c0, bool half) {
    const char* xc = reinterpret_cast<const char*>(x + c0 + 8 * (half ? gqh : gq));
#pragma unroll
    for (int q = 0; q < 4; ++q) raw[q] = *reinterpret_cast<const uint4*>(xc + t.o[q]);
  };
  auto combine = [&](bool half) -> uint4 {
    unsigned out[4];
#pragma unroll
    for (int wd = 0; wd < 4; ++wd) {
      u16 r[2];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int sh = 16 * hf;
        const unsigned q0 = wd == 0 ? raw[0].x : wd == 1 ? raw[0].y : wd == 2 ? raw[0].z : raw[0].w;
        const unsigned q1 = wd == 0 ? raw[1].x : wd == 1 ? raw[1].y : wd == 2 ? raw[1].z : raw[1].w;
        const unsigned q2 = wd == 0 ? raw[2].x : wd == 1 ? raw[2].y : wd == 2 ? raw[2].z : raw[2].w;
        const unsigned q3 = wd == 0 ? raw[3].x : wd == 1 ? raw[3].y : wd == 2 ? raw[3].z : raw[3].w;
        float v = t.w[0] * T::widen(static_cast<u16>((q0 >> sh) & 0xffffu));
        v = __builtin_fmaf(t.w[1], T::widen(static_cast<u16>((q1 >> sh) & 0xffffu)), v);
        v = __builtin_fmaf(t.w[2], T::widen(static_cast<u16>((q2 >> sh) & 0xffffu)), v);
        v = __builtin_fmaf(t.w[3], T::widen(static_cast<u16>((q3 >> sh) & 0xffffu)), v);
        r[hf] = T::round(v * t.m);
      }
      out[wd] = static_cast<unsigned>(r[0]) | (static_cast<unsigned>(r[1]) << 16);
    }
    if (half && upper) out[0] = out[1] = out[2] = out[3] = 0u;
    return make_uint4(out[0], out[1], out[2], out[3]);
  };
  f32x4 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // position of a step: tap k, deformable group dgi, chunk j of the group
  auto chan0 = [&](int dg_, int j_) { return dg_ * cpg + 32 * j_; };
  auto is_half = [&](int j_) { return tail && j_ == cps - 1; };
  // prologue: step 0 taps and operands; the offsets of the next (tap, group) segment
  load_offsets(0, 0);
  set_taps(0);
  if (g.dg > 1) load_offsets(0, 1);
  else if (K > 1) load_offsets(1, 0);
  dma(0, 0, is_half(0), lds_h);
  gather(0, is_half(0));
  uint4 bs = combine(is_half(0));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int k = 0, dgi = 0, j = 0;   // position of step s
  for (int s = 0; s < steps; ++s) {
    const uint4* cur = lds_h + (s & 1) * FRAG;
    // position of step s + 1
    int j1 = j + 1, dg1 = dgi, k1 = k;
    if (j1 == cps) { j1 = 0; if (++dg1 == g.dg) { dg1 = 0; ++k1; } }
    const bool more = s + 1 < steps;
    const bool new_seg = dg1 != dgi || k1 != k;   // the (tap, group) segment of step s + 1 starts there
    const bool half = is_half(j), half1 = is_half(j1);
    if (more) {
      if (new_seg) set_taps(k1);                  // its offsets were fetched a segment ago
      dma(k1, chan0(dg1, j1), half1, lds_h + ((s + 1) & 1) * FRAG);
      gather(chan0(dg1, j1), half1);
      if (new_seg) {                              // fetch the offsets of the segment after that
        int dg2 = dg1 + 1, k2 = k1;
        if (dg2 == g.dg) { dg2 = 0; ++k2; }
        if (k2 < K) load_offsets(k2, dg2);
      }
    }
    uint4 af[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) af[nb] = cur[nb * 64 + lane];
    if (half) {   // (uniform) the upper 16 channels of the step do not exist: zero in A as in B
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        if (upper) af[nb] = make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = T::mfma(af[nb], bs, acc[nb]);
    if (more) bs = combine(half1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    j = j1; dgi = dg1; k = k1;
  }
  // epilogue: acc[nb][reg] = y[pixel n][col0 + nb*16 + 4 gq + reg]
  if (!live) return;
  const bool vec = (g.Cout & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 7) == 0;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int col = col0 + nb * 16 + 4 * gq;
    if (col >= g.Cout) continue;
    u16 r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = T::round(acc[nb][e] + ((bias && col + e < g.Cout) ? bias[col + e] : 0.f));
    u16* dst = y + pix * g.Cout + col;
    if (vec && col + 3 < g.Cout) {
      *reinterpret_cast<uint2*>(dst) = make_uint2(static_cast<unsigned>(r[0]) | (static_cast<unsigned>(r[1]) << 16),
                                                  static_cast<unsigned>(r[2]) | (static_cast<unsigned>(r[3]) << 16));
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (col + e < g.Cout) dst[e] = r[e];
    }
  }
}

template <class T, int NB>
static void dcn_fwd_h_launch(const DcnGeom& g, const u16* x, const u16* wt_oc, const float* bias, const void* offset, const void* mask, int om16,
                             u16* y, long long npix, int col_blocks, hipStream_t stream) {
  const dim3 grid(static_cast<unsigned>(ceil_div(npix, 64) * col_blocks));   // one dimension: (tile, column block) decoded XCD-major in the kernel
  hipLaunchKernelGGL((dcn_fwd_h_k<T, NB>), grid, dim3(256), 2 * NB * 64 * sizeof(uint4), stream, g, x, wt_oc, bias, offset, mask, om16, y, col_blocks);
}

template <class T>
static int dcn_forward_h_run(const DcnGeom& g, const u16* x, const u16* wt_oc, const float* bias, const void* offset, const void* mask, int om16,
                             u16* y, hipStream_t stream) {
  const int bs = dcn_chunk_samples(g, false, 0, 2);
  FV2P_REQUIRE(bs >= 1, FV2P_ELIMIT, "dcn_forward_h: one sample's input is above 4 GiB");
  const long long K = static_cast<long long>(g.kh) * g.kw, pix = static_cast<long long>(g.Ho) * g.Wo;
  const long long om_bytes = om16 ? 2 : 4;
  const int nb_all = static_cast<int>(ceil_div(g.Cout, 16));
  for (int s0 = 0; s0 < g.B; s0 += bs) {
    DcnGeom gc = g;
    gc.B = std::min(bs, g.B - s0);
    const long long npix = static_cast<long long>(gc.B) * pix;
    const u16* xc = x + static_cast<long long>(s0) * g.H * g.W * g.Cin;
    const void* oc = static_cast<const char*>(offset) + static_cast<long long>(s0) * g.dg * 2 * K * pix * om_bytes;
    const void* mc = static_cast<const char*>(mask) + static_cast<long long>(s0) * g.dg * K * pix * om_bytes;
    u16* yc = y + static_cast<long long>(s0) * pix * g.Cout;
    // the plan of dcn_forward_run: 64 pixels x 16*NB columns per workgroup; 256 columns in one workgroup unless the map is too small
    // to fill the chip, then two column halves.  Per-pixel arithmetic does not depend on the plan.
    int nb = nb_all <= 4 ? 4 : (nb_all <= 8 ? 8 : 16);
    if (nb == 16 && ceil_div(npix, 64) < 2 * dcn_cu_count()) nb = 8;
    const int col_blocks = static_cast<int>(ceil_div(nb_all, nb));
    if (nb == 4) dcn_fwd_h_launch<T, 4>(gc, xc, wt_oc, bias, oc, mc, om16, yc, npix, col_blocks, stream);
    else if (nb == 8) dcn_fwd_h_launch<T, 8>(gc, xc, wt_oc, bias, oc, mc, om16, yc, npix, col_blocks, stream);
    else dcn_fwd_h_launch<T, 16>(gc, xc, wt_oc, bias, oc, mc, om16, yc, npix, col_blocks, stream);
  }
  FV2P_LAUNCH_CHECK();
  return 0;
}

}  // namespace fv2p
using namespace fv2p;

extern "C" int fv2p_dcn_forward_h_supported(int c_in, int c_out, int deformable_group) {
  return c_in >= 1 && c_out >= 1 && deformable_group >= 1 && c_in % deformable_group == 0 && (c_in / deformable_group) % 16 == 0;
}

extern "C" int fv2p_dcn_forward_h(const void* x_nhwc, const void* wt_oc, const float* bias, const void* offset, const void* mask,
                                  int batch, int height, int width, int c_in, int c_out, int h_out, int w_out, int kh, int kw,
                                  int sh, int sw, int ph, int pw, int dh, int dw, int deformable_group,
                                  void* y_nhwc, int dtype, int om_dtype, fv2p_stream_t stream_) {
  FV2P_DT16_OK("dcn_forward_h", dtype);
  FV2P_REQUIRE(om_dtype == 0 || om_dtype == dtype, FV2P_EINVAL, "dcn_forward_h: offset / mask dtype %d is neither fp32 (0) nor the call's dtype %d",
               om_dtype, dtype);
  const DcnGeom g = {batch, height, width, c_in, c_out, h_out, w_out, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group, 1};
  FV2P_REQUIRE(g.B >= 0 && g.H >= 1 && g.W >= 1 && g.Cin >= 1 && g.Cout >= 1 && g.kh >= 1 && g.kw >= 1 && g.sh >= 1 && g.sw >= 1 &&
                   g.dh >= 1 && g.dw >= 1 && g.dg >= 1 && g.Ho >= 1 && g.Wo >= 1,
               FV2P_EINVAL, "dcn_forward_h: bad geometry");
  FV2P_REQUIRE(fv2p_dcn_forward_h_supported(c_in, c_out, deformable_group), FV2P_ELIMIT,
               "dcn_forward_h: channels per deformable group (%d/%d) must be a multiple of 16", c_in, deformable_group);
  if (static_cast<long long>(g.B) * g.Ho * g.Wo == 0) return 0;
  FV2P_REQUIRE(x_nhwc && wt_oc && offset && mask && y_nhwc, FV2P_EINVAL, "dcn_forward_h: null pointer");
  FV2P_REQUIRE(aligned16(x_nhwc) && aligned16(wt_oc), FV2P_EINVAL, "dcn_forward_h: x and wt_oc must be 16-byte aligned");
  const u16* x = static_cast<const u16*>(x_nhwc);
  const u16* w = static_cast<const u16*>(wt_oc);
  u16* y = static_cast<u16*>(y_nhwc);
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (dtype == FV2P_DT_F16) return dcn_forward_h_run<DcnH16>(g, x, w, bias, offset, mask, om_dtype != 0, y, stream);
  return dcn_forward_h_run<DcnB16>(g, x, w, bias, offset, mask, om_dtype != 0, y, stream);
}
