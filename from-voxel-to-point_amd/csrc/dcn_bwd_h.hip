// A13 on float16 / bfloat16 maps: the backward of the modulated deformable convolution on v_mfma_f32_16x16x32_{f16,bf16}.
//
// The three passes of dcn.hip's backward in 16-bit storage: x NHWC [B,H,W,Cin], wt [K][Cin][Cout], dy [B*Ho*Wo][Cout], the column
// gradients colg [npix][K][Cin] of the workspace and dx NHWC hold 16-bit elements; no fp32 copy of a map exists.  grad_offset and
// grad_mask leave in the offsets' format (fp32 or the call's 16-bit format), the weight gradient dwt [K][Cin][Cout] in fp32.
//
//   dcn_bwd_col_h_k     dcol[p,k,ci] = sum_co wt[k][ci][co] dy[p][co]: A = weight rows (LDS-DMA, double buffer), B = dy of the wave's 16
//                       pixels, resident in registers (8 output channels per lane and fragment).  A step is (tap, 32 input channels): two
//                       A fragments whose rows are dealt so that a lane ends with EIGHT ADJACENT channels of its pixel - fragment f,
//                       row r = channel 8 (r >> 2) + 4 f + (r & 3); C/D row 4 gq + e of fragment f is then channel 8 gq + 4 f + e.  The
//                       lane fetches the same eight channels of x at the four corners (16 bytes each), adds <dcol, x[corner]> to its four
//                       D_q in fp32 from the fp32 accumulators, and stores colg = round(dcol * mask) as 16 bytes.  At the end of a
//                       (tap, deformable group) segment D_q is summed over the four lane quarters and grad_mask / grad_offset are written
//                       ONCE with dcn_bwd_col_k's formulas (Cout <= 256: no slices, nothing is added in place).
//   dcn_col2im_h_k      the gather of dcn_col2im_k over the same sample lists (dcn.hip builds them from offsets of either format): 16-bit
//                       colg rows, fp32 sums in the same key and sample order, one rounding into dx.  No atomics, no zero fill.
//   dcn_bwd_weight_h_k  dW[k][ci][co] = sum_p col[p,k,ci] dy[p,co], col formed as the forward forms its B operand (widened corners, the
//                       fmaf chain, times the mask, one rounding).  The MFMA's k index is the PIXEL: both tiles are staged in LDS
//                       channel-major, a thread writing two adjacent pixels of a channel as one dword, so that a lane's 8 consecutive
//                       pixels of one channel are one 16-byte row piece (two ds_read_b64).  fp32 partials per pixel split, folded in
//                       ascending order by dcn_reduce_k.
//
// A deformable group 16 mod 32 wide ends in a 16-channel step.  Its A rows 8 .. 15 of both fragments (channels 16 .. 31 of the step) do
// not exist: those lanes hand the LDS-DMA the addresses of rows 0 .. 7 and the operand is replaced by zeros after the LDS read; the
// lanes gq >= 2, whose C/D rows those are, fetch x where the lanes gq - 2 do, add nothing to D_q and store nothing.  Output channels
// past Cout (Cout = 8 mod 32 ...) are zero in BOTH operands, the weight address clamped into the row.  Nothing outside x, wt or dy is read,
// and no product 0 x (anything) reaches a value that is kept.
#include "common.hpp"
#include "dcn_common.hpp"
#include "dt16.hpp"
#include <stdlib.h>
#include <algorithm>

namespace fv2p {

using f16x8 = _Float16 __attribute__((ext_vector_type(8)));
using bf16x8 = __bf16 __attribute__((ext_vector_type(8)));

struct BwdH16 : H16 {
  static constexpr int code = FV2P_DT_F16;
  static __device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};
struct BwdB16 : B16 {
  static constexpr int code = FV2P_DT_BF16;
  static __device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};

// offset / mask element i: fp32 (om16 == 0) or the call's 16-bit format; the gradients leave the same way, rounded once
template <class T>
__device__ __forceinline__ float om_get(const void* p, long long i, int om16) {
  return om16 ? T::widen(static_cast<const u16*>(p)[i]) : static_cast<const float*>(p)[i];
}
template <class T>
__device__ __forceinline__ void om_put(void* p, long long i, int om16, float v) {
  if (om16) static_cast<u16*>(p)[i] = T::round(v);
  else static_cast<float*>(p)[i] = v;
}

// element e (0 .. 7) of a 16-byte piece of 16-bit values, widened
template <class T>
__device__ __forceinline__ float piece_elem(const uint4& q, int e) {
  const unsigned w = (e >> 1) == 0 ? q.x : (e >> 1) == 1 ? q.y : (e >> 1) == 2 ? q.z : q.w;
  return T::widen(static_cast<u16>((w >> (16 * (e & 1))) & 0xffffu));
}
template <class T>
__device__ __forceinline__ uint4 piece_round(const float (&v)[8]) {
  unsigned w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = static_cast<unsigned>(T::round(v[2 * i])) | (static_cast<unsigned>(T::round(v[2 * i + 1])) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// ---------------------------------------------------------------- pass 1: column gradients, grad_mask, grad_offset -------------------
// JB = ceil(Cout / 32) rounded up to 1, 2, 4 or 8: dy fragments of 32 output channels.  Block = 4 waves, wave = 16 pixels; n_share
// workgroups share the (tap, deformable group) segments of a pixel tile in equal parts (dcn_bwd_col_k's seg_split).
template <class T, int JB>
__global__ __launch_bounds__(256, 2) void dcn_bwd_col_h_k(DcnGeom g, const u16* __restrict__ x, const u16* __restrict__ wt,
                                                           const void* __restrict__ offset, const void* __restrict__ mask, int om16,
                                                           const u16* __restrict__ dy, u16* __restrict__ colg, void* __restrict__ doff,
                                                           void* __restrict__ dmask, int n_share) {
  extern __shared__ __attribute__((aligned(16))) uint4 lds_c[];   // 2 x (2 JB) pieces of 64 x 16 bytes
  constexpr int NP = 2 * JB, FRAG = NP * 64, NDMA = (NP + 3) / 4;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n = lane & 15, gq = lane >> 4;
  const long long npix = static_cast<long long>(g.B) * g.Ho * g.Wo;
  const int plane = g.Ho * g.Wo;
  const int K = g.kh * g.kw, cpg = g.Cin / g.dg, cps = (cpg + 31) / 32;
  const bool tail = (cpg & 31) != 0;   // cpg = 16 mod 32
  long long tile;
  int share;
  xcd_tile(n_share, tile, share);
  // segment sg = (tap sg / dg, deformable group sg % dg); this workgroup's segments [seg_begin, seg_end)
  const int segs = K * g.dg;
  const int seg_begin = static_cast<int>(static_cast<long long>(segs) * share / n_share);
  const int seg_end = static_cast<int>(static_cast<long long>(segs) * (share + 1) / n_share);
  const int steps = (seg_end - seg_begin) * cps;
  if (steps <= 0) return;
  const long long pix = tile * 64 + wave * 16 + n;
  const bool live = pix < npix;
  const long long pp = live ? pix : 0;
  const int pb = static_cast<int>(pp / plane), ppos = static_cast<int>(pp % plane), pho = ppos / g.Wo, pwo = ppos % g.Wo;
  const unsigned cbase = static_cast<unsigned>(pp * K * g.Cin * 2);   // byte offset of colg[p][0][0] (the chunk rule keeps it below 2^32)
  const bool upper = gq >= 2;
  // dy of the pixel: fragment jb, lane (n, gq) = output channels 32 jb + 8 gq .. + 7, zero past Cout and for a pixel past the end
  uint4 dyr[JB];
  bool co_out[JB];   // the lane's 8 output channels of fragment jb do not exist: zero in A as in B
#pragma unroll
  for (int jb = 0; jb < JB; ++jb) {
    const int co = 32 * jb + 8 * gq;
    co_out[jb] = co >= g.Cout;   // Cout % 8 == 0: a piece is inside or outside as a whole
    dyr[jb] = (live && !co_out[jb]) ? *reinterpret_cast<const uint4*>(dy + pp * g.Cout + co) : make_uint4(0u, 0u, 0u, 0u);
  }
  // LDS-DMA: piece (f, jb), lane (n, gq) <- wt[k][c0 + 8 (n' >> 2) + 4 f + (n' & 3)][32 jb + 8 gq ..], n' = n (n & 7 in a 16-channel step)
  auto dma = [&](int k, int c0, bool half, uint4* buf) {
    const int nr = half ? (n & 7) : n;
#pragma unroll
    for (int i = 0; i < NDMA; ++i) {
      const int pc = wave + 4 * i;
      if (pc < NP) {
        const int f = pc / JB, jb = pc % JB;
        const int ch = c0 + 8 * (nr >> 2) + 4 * f + (nr & 3);
        const int co = min(32 * jb + 8 * gq, g.Cout - 8);
        glds16(wt + (static_cast<long long>(k) * g.Cin + ch) * g.Cout + co, buf + pc * 64);
      }
    }
  };
  CornerB t;
  float roh, row_, rom;   // raw offsets / mask of the NEXT segment
  auto load_offsets = [&](int k, int dgi) {
    const long long ob = (static_cast<long long>(pb) * g.dg + dgi) * 2 * K * plane + ppos;
    roh = om_get<T>(offset, ob + static_cast<long long>(2 * k) * plane, om16);
    row_ = om_get<T>(offset, ob + static_cast<long long>(2 * k + 1) * plane, om16);
    rom = om_get<T>(mask, ((static_cast<long long>(pb) * g.dg + dgi) * K + k) * plane + ppos, om16);
  };
  auto set_taps = [&](int k) {
    const int i = k / g.kw, j = k % g.kw;
    const float h_im = static_cast<float>(pho * g.sh - g.ph + i * g.dh) + roh;
    const float w_im = static_cast<float>(pwo * g.sw - g.pw + j * g.dw) + row_;
    make_corners_b<2>(g, live, pb, h_im, w_im, rom, 0u, t);
  };
  float Dq[4] = {0.f, 0.f, 0.f, 0.f};
  int sg = seg_begin, j = 0;   // segment and 32-channel chunk of step s
  load_offsets(sg / g.dg, sg % g.dg);
  set_taps(sg / g.dg);
  if (sg + 1 < seg_end) load_offsets((sg + 1) / g.dg, (sg + 1) % g.dg);
  dma(sg / g.dg, (sg % g.dg) * cpg, tail && cps == 1, lds_c);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const uint4* cur = lds_c + (s & 1) * FRAG;
    const int k = sg / g.dg, dgi = sg % g.dg;
    int j1 = j + 1, sg1 = sg;
    if (j1 == cps) { j1 = 0; ++sg1; }
    const bool more = s + 1 < steps;
    const bool half = tail && j == cps - 1;
    const int c0 = dgi * cpg + 32 * j;
    if (more) dma(sg1 / g.dg, (sg1 % g.dg) * cpg + 32 * j1, tail && j1 == cps - 1, lds_c + ((s + 1) & 1) * FRAG);
    // x at the four corners: the lane's eight channels c0 + 8 gq .. + 7 (a 16-channel step: the lanes gq >= 2 fetch where gq - 2 does)
    uint4 raw[4];
    {
      const char* xc = reinterpret_cast<const char*>(x + c0 + 8 * (half ? (gq & 1) : gq));
#pragma unroll
      for (int q = 0; q < 4; ++q) raw[q] = *reinterpret_cast<const uint4*>(xc + t.o[q]);
    }
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const bool row_out = half && n >= 8;   // this lane's A row does not exist
#pragma unroll
    for (int jb = 0; jb < JB; ++jb) {
      uint4 a0 = cur[jb * 64 + lane], a1 = cur[(JB + jb) * 64 + lane];
      if (row_out || co_out[jb]) a0 = a1 = make_uint4(0u, 0u, 0u, 0u);
      acc[0] = T::mfma(a0, dyr[jb], acc[0]);
      acc[1] = T::mfma(a1, dyr[jb], acc[1]);
    }
    // acc[f][e] = dcol[pixel n][c0 + 8 gq + 4 f + e]
    const bool mine = !(half && upper);
    {
      float d[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) { d[e] = acc[0][e]; d[4 + e] = acc[1][e]; }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float a = Dq[q];
#pragma unroll
        for (int e = 0; e < 8; ++e) a = __builtin_fmaf(d[e], piece_elem<T>(raw[q], e), a);
        Dq[q] = mine ? a : Dq[q];
      }
      if (live && mine) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = d[e] * t.m;
        char* dst = reinterpret_cast<char*>(colg + (static_cast<long long>(k) * g.Cin + c0 + 8 * gq));
        *reinterpret_cast<uint4*>(dst + cbase) = piece_round<T>(v);
      }
    }
    if (sg1 != sg || !more) {
      // end of the (tap, group) segment: D_q over the four channel quarters (lanes n, n + 16, n + 32, n + 48), grad_mask / grad_offset
      float D[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float a = Dq[q];
        a += __shfl_xor(a, 16, 64);
        a += __shfl_xor(a, 32, 64);
        D[q] = (t.vb >> q) & 1u ? a : 0.f;
        Dq[q] = 0.f;
      }
      if (gq == 0 && live) {
        const float lh = t.lh, lw = t.lw, hh = 1.f - lh, hw = 1.f - lw, m = t.m;
        const float gm = t.w[0] * D[0] + t.w[1] * D[1] + t.w[2] * D[2] + t.w[3] * D[3];
        const float gh = m * (-hw * D[0] - lw * D[1] + hw * D[2] + lw * D[3]);
        const float gw = m * (-hh * D[0] + hh * D[1] - lh * D[2] + lh * D[3]);
        const long long ob = (static_cast<long long>(pb) * g.dg + dgi) * 2 * K * plane + ppos;
        om_put<T>(dmask, ((static_cast<long long>(pb) * g.dg + dgi) * K + k) * plane + ppos, om16, gm);
        om_put<T>(doff, ob + static_cast<long long>(2 * k) * plane, om16, gh);
        om_put<T>(doff, ob + static_cast<long long>(2 * k + 1) * plane, om16, gw);
      }
      if (more) {
        set_taps(sg1 / g.dg);   // its offsets were fetched a segment ago
        if (sg1 + 1 < seg_end) load_offsets((sg1 + 1) / g.dg, (sg1 + 1) % g.dg);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    j = j1; sg = sg1;
  }
}

// ---------------------------------------------------------------- pass 2: grad_input in gather form ----------------------------------
template <class T, int VEC>
__device__ __forceinline__ void colh_load(const u16* p, float (&v)[VEC]) {
  if constexpr (VEC == 8) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = piece_elem<T>(q, e);
  } else if constexpr (VEC == 4) {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
    v[0] = T::widen(static_cast<u16>(q.x & 0xffffu)); v[1] = T::widen(static_cast<u16>(q.x >> 16));
    v[2] = T::widen(static_cast<u16>(q.y & 0xffffu)); v[3] = T::widen(static_cast<u16>(q.y >> 16));
  } else if constexpr (VEC == 2) {
    const unsigned q = *reinterpret_cast<const unsigned*>(p);
    v[0] = T::widen(static_cast<u16>(q & 0xffffu)); v[1] = T::widen(static_cast<u16>(q >> 16));
  } else {
    v[0] = T::widen(p[0]);
  }
}

// dcn_col2im_k on 16-bit column gradients: one wave per (2 x 4 tile of input pixels, sample, deformable group), lane = VEC adjacent
// channels of the group; keys, lists and sample order as there; fp32 sums, one rounding into dx
template <class T, int VEC>
__global__ __launch_bounds__(256) void dcn_col2im_h_k(DcnGeom g, const u16* __restrict__ colg, const int* __restrict__ ends, DcnEntries en,
                                                      u16* __restrict__ dx) {
  __shared__ unsigned s_src[4][64];
  __shared__ float s_lh[4][64], s_lw[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles_c = (g.W + 3) / 4, tiles_r = (g.H + 1) / 2;
  const long long ntiles = static_cast<long long>(g.B) * g.dg * tiles_r * tiles_c;
  long long blk;
  int unused;
  xcd_tile(1, blk, unused);
  const long long tile = blk * 4 + wave;
  if (tile >= ntiles) return;
  const int cpg = g.Cin / g.dg;
  const int bd = static_cast<int>(tile / (tiles_r * tiles_c)), b = bd / g.dg, dgi = bd % g.dg;
  const int tr0 = static_cast<int>((tile / tiles_c) % tiles_r) * 2, tc0 = static_cast<int>(tile % tiles_c) * 4;
  const int nl = min(5, g.W + 1 - tc0);   // key columns tc0 .. tc0 + nl - 1 exist
  unsigned* ssrc = s_src[wave];
  float *slh = s_lh[wave], *slw = s_lw[wave];
  for (int c0 = 0; c0 < cpg; c0 += 64 * VEC) {
    const int c = c0 + lane * VEC;
    const bool act = c < cpg;
    const u16* col = colg + static_cast<long long>(dgi) * cpg + (act ? c : 0);
    float acc[2][4][VEC];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[a][e][v] = 0.f;
    auto add = [&](auto I_, auto J_, float lh, float lw, const float (&row)[VEC]) {
      constexpr int I = decltype(I_)::value, J = decltype(J_)::value;
      const float hh = 1.f - lh, hw = 1.f - lw;
#pragma unroll
      for (int dr = 0; dr < 2; ++dr)
#pragma unroll
        for (int dc = 0; dc < 2; ++dc) {
          const int tr = I - 1 + dr, tc = J - 1 + dc;
          if (tr < 0 || tr > 1 || tc < 0 || tc > 3) continue;
          const float w = (dr ? lh : hh) * (dc ? lw : hw);
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[tr][tc][v] = __builtin_fmaf(w, row[v], acc[tr][tc][v]);
        }
    };
    // entries [lo, hi) of the wave's LDS stage belong to key (I, J)
    auto walk = [&](auto I_, auto J_, int lo, int hi) {
      int e = lo;
      for (; e + 2 <= hi; e += 2) {
        unsigned s[2]; float a[2], bq[2]; float r[2][VEC];
#pragma unroll
        for (int u = 0; u < 2; ++u) { s[u] = ssrc[e + u]; a[u] = slh[e + u]; bq[u] = slw[e + u]; }
#pragma unroll
        for (int u = 0; u < 2; ++u) colh_load<T, VEC>(col + static_cast<long long>(s[u]) * g.Cin, r[u]);
#pragma unroll
        for (int u = 0; u < 2; ++u) add(I_, J_, a[u], bq[u], r[u]);
      }
      for (; e < hi; ++e) {
        float r[VEC];
        colh_load<T, VEC>(col + static_cast<long long>(ssrc[e]) * g.Cin, r);
        add(I_, J_, slh[e], slw[e], r);
      }
    };
    auto key_row = [&](auto I_) {
      constexpr int I = decltype(I_)::value;
      const int kr = tr0 + I;   // key row; exists for kr <= H
      if (kr > g.H) return;
      const long long kbase = (static_cast<long long>(bd) * (g.H + 1) + kr) * (g.W + 1) + tc0;
      // list bounds of the nl keys: s[j] = end of key kbase + j - 1 (= start of key kbase + j)
      int bound = 0;
      if (lane <= nl) { const long long kk = kbase + lane - 1; bound = kk >= 0 ? ends[kk] : 0; }
      int s[6];
#pragma unroll
      for (int jj = 0; jj < 6; ++jj) s[jj] = __shfl(bound, min(jj, nl), 64);
      const int run0 = s[0], nrun = s[5] - s[0];
      if (nrun <= 64) {
        // the five lists are one contiguous run: rank every entry by (list, sample) inside the wave
        unsigned src = 0xffffffffu; float lh = 0.f, lw = 0.f;
        int mylist = 8;
        if (lane < nrun) {
          src = en.src[run0 + lane]; lh = en.lh[run0 + lane]; lw = en.lw[run0 + lane];
          mylist = 0;
#pragma unroll
          for (int jj = 1; jj < 5; ++jj) mylist += (run0 + lane >= s[jj]);
        }
        const unsigned long long mine = (static_cast<unsigned long long>(mylist) << 32) | src;
        int rank = 0;
        for (int jj = 0; jj < nrun; ++jj) {
          const unsigned long long o = (static_cast<unsigned long long>(static_cast<unsigned>(__shfl(mylist, jj, 64))) << 32) |
                                       static_cast<unsigned>(__shfl(static_cast<int>(src), jj, 64));
          rank += o < mine;
        }
        if (lane < nrun) { ssrc[rank] = src; slh[rank] = lh; slw[rank] = lw; }
        // (one wave, in-order LDS: no barrier)
        walk(I_, std::integral_constant<int, 0>{}, s[0] - run0, s[1] - run0);
        walk(I_, std::integral_constant<int, 1>{}, s[1] - run0, s[2] - run0);
        walk(I_, std::integral_constant<int, 2>{}, s[2] - run0, s[3] - run0);
        walk(I_, std::integral_constant<int, 3>{}, s[3] - run0, s[4] - run0);
        walk(I_, std::integral_constant<int, 4>{}, s[4] - run0, s[5] - run0);
      } else {
        auto one = [&](auto J_, int lo, int hi) {
          const int nn = hi - lo;
          for (int base = 0; base < nn; base += 64) {
            const int cnt = min(64, nn - base);
            unsigned src = 0xffffffffu; float lh = 0.f, lw = 0.f;
            if (lane < cnt) { src = en.src[lo + base + lane]; lh = en.lh[lo + base + lane]; lw = en.lw[lo + base + lane]; }
            int rank = lane;                                   // lists above 64 entries were sorted by dcn_index_sort_long_k
            if (nn <= 64) {
              rank = 0;
              for (int jj = 0; jj < cnt; ++jj) rank += static_cast<unsigned>(__shfl(static_cast<int>(src), jj, 64)) < src;
            }
            if (lane < cnt) { ssrc[rank] = src; slh[rank] = lh; slw[rank] = lw; }
            walk(I_, J_, 0, cnt);
          }
        };
        one(std::integral_constant<int, 0>{}, s[0], s[1]);
        one(std::integral_constant<int, 1>{}, s[1], s[2]);
        one(std::integral_constant<int, 2>{}, s[2], s[3]);
        one(std::integral_constant<int, 3>{}, s[3], s[4]);
        one(std::integral_constant<int, 4>{}, s[4], s[5]);
      }
    };
    key_row(std::integral_constant<int, 0>{});
    key_row(std::integral_constant<int, 1>{});
    key_row(std::integral_constant<int, 2>{});
    if (act) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = tr0 + a, cc = tc0 + e;
          if (r >= g.H || cc >= g.W) continue;
          u16* out = dx + ((static_cast<long long>(b) * g.H + r) * g.W + cc) * g.Cin + dgi * cpg + c;
          if constexpr (VEC == 8) *reinterpret_cast<uint4*>(out) = piece_round<T>(acc[a][e]);
          else if constexpr (VEC == 4)
            *reinterpret_cast<uint2*>(out) = make_uint2(static_cast<unsigned>(T::round(acc[a][e][0])) | (static_cast<unsigned>(T::round(acc[a][e][1])) << 16),
                                                        static_cast<unsigned>(T::round(acc[a][e][2])) | (static_cast<unsigned>(T::round(acc[a][e][3])) << 16));
          else if constexpr (VEC == 2)
            *reinterpret_cast<unsigned*>(out) = static_cast<unsigned>(T::round(acc[a][e][0])) | (static_cast<unsigned>(T::round(acc[a][e][1])) << 16);
          else out[0] = T::round(acc[a][e][0]);
        }
    }
  }
}

// ---------------------------------------------------------------- pass 3: weight gradient --------------------------------------------
// One workgroup = (pixel range, tap, 128 input channels, 128 output channels); a step is 32 pixels.  Thread (pair = tid & 15, oct =
// tid >> 4) builds col for the pixels 2 pair, 2 pair + 1 of the step and the channels ci0 + 8 oct .. + 7 (four 16-byte corner loads per
// pixel, the forward's combine) and fetches dy of the same pixels, columns co0 + 8 oct .. + 7; both go to LDS CHANNEL-MAJOR, one dword =
// (pixel 2 pair, pixel 2 pair + 1) of one channel, rows of kDwhPitch dwords.  A wave multiplies its 64 x 64 corner of the tile: A[ci][px]
// and B[px][co], a lane's 8 consecutive pixels of a channel being 16 bytes of one row (two ds_read_b64; a row pitch of 18 dwords is no
// multiple of 16 bytes).  Banks: a write's 32-lane half holds 16 pairs x 2 octets, dword (8 oct + c) 18 + pair: 8 * 18 = 16 mod 32, the
// two octets fill opposite halves of the 32 banks - no conflict.  A read's half holds rows r = 0 .. 15 and gq = 0, 1 at dword 18 r + 4 gq
// (+ 0, 1): 18 r mod 64 are 16 distinct even banks, and + 4 meets them only at (r, r') = (14, 0), (15, 1): two 2-way pairs per read,
// which no even pitch with conflict-free writes avoids (18 d = 4 mod 64 always has a solution |d| < 16).
constexpr int kDwhPitch = 18;                 // dwords per channel row of an LDS tile: 16 of pixels + 2 of padding
constexpr int kDwhTile = 128 * kDwhPitch;     // dwords of one tile (col or dy)
template <class T>
__global__ __launch_bounds__(256, 2) void dcn_bwd_weight_h_k(DcnGeom g, const u16* __restrict__ x, const void* __restrict__ offset,
                                                              const void* __restrict__ mask, int om16, const u16* __restrict__ dy,
                                                              int pix_per_block, int n_ztiles, float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) unsigned lds_w[2 * 2 * kDwhTile];   // 2 buffers x (col tile, dy tile)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 15, gq = lane >> 4;
  const int K = g.kh * g.kw, cpg = g.Cin / g.dg, plane = g.Ho * g.Wo;
  const int ci_tiles = (g.Cin + 127) / 128;
  long long lp;
  int zt;
  xcd_tile(n_ztiles, lp, zt);
  const int k = static_cast<int>(lp % K), split = static_cast<int>(lp / K);
  const int ci0 = (zt % ci_tiles) * 128, co0 = (zt / ci_tiles) * 128;
  const long long npix = static_cast<long long>(g.B) * plane;
  const long long p_begin = static_cast<long long>(split) * pix_per_block, p_end = min(p_begin + pix_per_block, npix);
  const int pair = tid & 15, oct = tid >> 4;
  const int ci = ci0 + 8 * oct, co = co0 + 8 * oct;
  const bool ci_ok = ci < g.Cin, co_ok = co < g.Cout;        // Cin % 16 == 0, Cout % 8 == 0: an octet is inside or outside as a whole
  const int cia = ci_ok ? ci : 0, dgi = cia / cpg;           // an octet never crosses a deformable group (cpg % 16 == 0)
  const int i_k = k / g.kw, j_k = k % g.kw;
  uint4 raw[2][4], dyv[2];
  float wq[2][4], mk[2];
  bool okp[2];
  float roh[2], row_[2], rom[2];
  auto load_offsets = [&](long long p0) {   // raw offsets / mask of the thread's two pixels
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long long p = p0 + h;
      const long long pp = p < p_end ? p : p_begin;
      const int b = static_cast<int>(pp / plane), pos = static_cast<int>(pp % plane);
      const long long ob = (static_cast<long long>(b) * g.dg + dgi) * 2 * K * plane + pos;
      roh[h] = om_get<T>(offset, ob + static_cast<long long>(2 * k) * plane, om16);
      row_[h] = om_get<T>(offset, ob + static_cast<long long>(2 * k + 1) * plane, om16);
      rom[h] = om_get<T>(mask, ((static_cast<long long>(b) * g.dg + dgi) * K + k) * plane + pos, om16);
    }
  };
  auto issue = [&](long long p0) {   // corner loads + dy loads of the two pixels (taps from the raw offsets fetched one step earlier)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long long p = p0 + h;
      const bool ok = p < p_end;
      const long long pp = ok ? p : p_begin;
      const int b = static_cast<int>(pp / plane), pos = static_cast<int>(pp % plane);
      const int ho = pos / g.Wo, wo = pos % g.Wo;
      Corner4 t;
      const float h_im = static_cast<float>(ho * g.sh - g.ph + i_k * g.dh) + roh[h];
      const float w_im = static_cast<float>(wo * g.sw - g.pw + j_k * g.dw) + row_[h];
      make_corners<2>(g, ok && ci_ok, b, h_im, w_im, rom[h], static_cast<unsigned>(cia) * 2u, t);
#pragma unroll
      for (int q = 0; q < 4; ++q) { raw[h][q] = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(x) + t.o[q]); wq[h][q] = t.w[q]; }
      mk[h] = t.m;
      okp[h] = ok && ci_ok;
      dyv[h] = (ok && co_ok) ? *reinterpret_cast<const uint4*>(dy + pp * g.Cout + co) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto stage = [&](unsigned* buf) {   // combine + write both tiles, channel-major, two pixels per dword
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      unsigned cw = 0u, dw = 0u;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float v = wq[h][0] * piece_elem<T>(raw[h][0], e);
        v = __builtin_fmaf(wq[h][1], piece_elem<T>(raw[h][1], e), v);
        v = __builtin_fmaf(wq[h][2], piece_elem<T>(raw[h][2], e), v);
        v = __builtin_fmaf(wq[h][3], piece_elem<T>(raw[h][3], e), v);
        const u16 cv = okp[h] ? T::round(v * mk[h]) : static_cast<u16>(0);   // a pixel past the range or a channel past Cin: zero, not 0 x (x)
        cw |= static_cast<unsigned>(cv) << (16 * h);
        const unsigned dq = (e >> 1) == 0 ? dyv[h].x : (e >> 1) == 1 ? dyv[h].y : (e >> 1) == 2 ? dyv[h].z : dyv[h].w;
        dw |= ((dq >> (16 * (e & 1))) & 0xffffu) << (16 * h);
      }
      buf[(8 * oct + e) * kDwhPitch + pair] = cw;
      buf[kDwhTile + (8 * oct + e) * kDwhPitch + pair] = dw;
    }
  };
  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int wi = wave >> 1, wj = wave & 1;
  const long long steps = (p_end - p_begin + 31) / 32;
  if (steps > 0) {
    load_offsets(p_begin + 2 * pair);
    issue(p_begin + 2 * pair);
    if (steps > 1) load_offsets(p_begin + 32 + 2 * pair);
    stage(lds_w);
  }
  __syncthreads();
  for (long long s = 0; s < steps; ++s) {
    const unsigned* cur = lds_w + (s & 1) * (2 * kDwhTile);
    const bool more = s + 1 < steps;
    if (more) {
      issue(p_begin + (s + 1) * 32 + 2 * pair);
      if (s + 2 < steps) load_offsets(p_begin + (s + 2) * 32 + 2 * pair);
    }
    uint4 av[4], bv[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const uint2* p = reinterpret_cast<const uint2*>(cur + ((wi * 4 + a) * 16 + r) * kDwhPitch + 4 * gq);
      const uint2 lo = p[0], hi = p[1];
      av[a] = make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint2* p = reinterpret_cast<const uint2*>(cur + kDwhTile + ((wj * 4 + c) * 16 + r) * kDwhPitch + 4 * gq);
      const uint2 lo = p[0], hi = p[1];
      bv[c] = make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[a][c] = T::mfma(av[a], bv[c], acc[a][c]);
    if (more) stage(lds_w + ((s + 1) & 1) * (2 * kDwhTile));
    __syncthreads();
  }
  // acc[a][c][e] = dW[k][ci0 + (wi*4 + a)*16 + 4 gq + e][co0 + (wj*4 + c)*16 + r]
  float* out = partial + (static_cast<long long>(split) * K + k) * g.Cin * g.Cout;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int cio = ci0 + (wi * 4 + a) * 16 + 4 * gq + e;
      if (cio >= g.Cin) continue;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int coo = co0 + (wj * 4 + c) * 16 + r;
        if (coo < g.Cout) out[static_cast<long long>(cio) * g.Cout + coo] = acc[a][c][e];
      }
    }
}

// ---------------------------------------------------------------- host ---------------------------------------------------------------
constexpr long long kDwhBlocksPerCu = 2;   // workgroups of the weight-gradient kernel per CU: __launch_bounds__(256, 2), 36 KB of LDS each
struct DcnBwdHPlan {
  long long npix, nkeys, max_entries;
  int splits, pix_per_block, ci_tiles, co_tiles, splits_cap;
};
static DcnBwdHPlan dcn_bwd_h_plan(const DcnGeom& g) {
  DcnBwdHPlan p;
  const int K = g.kh * g.kw;
  p.npix = static_cast<long long>(g.B) * g.Ho * g.Wo;
  p.nkeys = static_cast<long long>(g.B) * g.dg * (g.H + 1) * (g.W + 1);
  p.max_entries = p.npix * g.dg * K;
  p.ci_tiles = static_cast<int>(ceil_div(g.Cin, 128));
  p.co_tiles = static_cast<int>(ceil_div(g.Cout, 128));
  const long long cols = static_cast<long long>(K) * p.ci_tiles * p.co_tiles;
  const long long npx = p.npix > 0 ? p.npix : 1;
  // one resident round of workgroups, at least 64 pixels each (dcn_bwd_plan's rule); a range is whole 32-pixel steps
  const long long cap = std::max<long long>(1, std::min<long long>((kDwhBlocksPerCu * dcn_cu_count()) / cols, ceil_div(npx, 64)));
  const long long ppb = ceil_div(ceil_div(npx, cap), 32) * 32;
  p.pix_per_block = static_cast<int>(ppb);
  p.splits = static_cast<int>(ceil_div(npx, ppb));
  p.splits_cap = static_cast<int>(cap);   // splits <= cap whatever the sample count: what `partial` is carved for
  return p;
}
template <typename C>
static void dcn_bwd_h_carve(C& c, const DcnGeom& g, const DcnBwdHPlan& p, u16** colg, int** cursor, DcnEntries* entries, void** scan_ws,
                            float** partial) {
  const int K = g.kh * g.kw;
  *colg = c.template take<u16>(static_cast<size_t>(p.npix) * K * g.Cin);
  *cursor = c.template take<int>(static_cast<size_t>(p.nkeys) + 1);
  entries->src = c.template take<unsigned>(static_cast<size_t>(p.max_entries));
  entries->lh = c.template take<float>(static_cast<size_t>(p.max_entries));
  entries->lw = c.template take<float>(static_cast<size_t>(p.max_entries));
  *scan_ws = c.template take<char>(scan_ws_bytes(p.nkeys));
  *partial = c.template take<float>(static_cast<size_t>(p.splits_cap) * K * g.Cin * g.Cout);
}

static size_t dcn_backward_h_ws(DcnGeom g) {
  g.B = std::max(1, std::min(g.B, dcn_chunk_samples(g, true, dcn_colg_cap(), 2)));   // the workspace of one chunk serves every chunk
  const DcnBwdHPlan p = dcn_bwd_h_plan(g);
  SizerC s;
  u16* a; float* e; int* b; DcnEntries c; void* d;
  dcn_bwd_h_carve(s, g, p, &a, &b, &c, &d, &e);
  return s.bytes();
}

template <class T, int JB>
static void dcn_col_h_launch(const DcnGeom& g, const u16* x, const u16* wt, const void* offset, const void* mask, int om16, const u16* dy, u16* colg,
                             void* doff, void* dmask, long long npix, int seg_split, hipStream_t stream) {
  hipLaunchKernelGGL((dcn_bwd_col_h_k<T, JB>), dim3(static_cast<unsigned>(ceil_div(npix, 64) * seg_split)), dim3(256),
                     2 * 2 * JB * 64 * sizeof(uint4), stream, g, x, wt, offset, mask, om16, dy, colg, doff, dmask, seg_split);
}

template <class T, int VEC>
static void dcn_col2im_h_launch(const DcnGeom& g, const u16* colg, const int* cursor, DcnEntries entries, u16* dx, hipStream_t stream) {
  const long long ntiles = static_cast<long long>(g.B) * g.dg * ((g.H + 1) / 2) * ((g.W + 3) / 4);
  hipLaunchKernelGGL((dcn_col2im_h_k<T, VEC>), dim3(static_cast<unsigned>(ceil_div(ntiles, 4))), dim3(256), 0, stream, g, colg, cursor, entries, dx);
}

// dx_nhwc, doffset, dmask, dwt are fully written (nothing to zero).  wt = [kh*kw][Cin][Cout] in T, dwt likewise in fp32.
template <class T>
static int dcn_backward_h_run(const DcnGeom& g, const u16* x_nhwc, const u16* wt, const void* offset, const void* mask, const u16* dy_nhwc,
                              u16* dx_nhwc, void* doffset, void* dmask, float* dwt, void* ws, size_t ws_bytes, int om16, hipStream_t stream) {
  const long long pix = static_cast<long long>(g.Ho) * g.Wo, npix = g.B * pix;
  const int K = g.kh * g.kw;
  FV2P_REQUIRE(dwt, FV2P_EINVAL, "dcn_backward_h: null dwt");
  if (npix == 0) {   // an empty batch (Ho, Wo >= 1): the weight gradient is zero and no other output has an element
    FV2P_HIP(hipMemsetAsync(dwt, 0, sizeof(float) * (size_t)K * g.Cin * g.Cout, stream));
    return 0;
  }
  FV2P_REQUIRE(x_nhwc && wt && offset && mask && dy_nhwc && dx_nhwc && doffset && dmask, FV2P_EINVAL, "dcn_backward_h: null pointer");
  FV2P_REQUIRE(aligned16(x_nhwc) && aligned16(wt) && aligned16(dy_nhwc) && aligned16(dx_nhwc), FV2P_EINVAL,
               "dcn_backward_h: x, wt, dy and dx must be 16-byte aligned");
  const int bs = dcn_chunk_samples(g, true, dcn_colg_cap(), 2);
  FV2P_REQUIRE(bs >= 1, FV2P_ELIMIT, "dcn_backward_h: one sample's input, column gradients or sample list is above the 32-bit limits");
  FV2P_REQUIRE(ws && ws_bytes >= dcn_backward_h_ws(g), FV2P_EWORKSPACE, "dcn_backward_h: workspace too small");
  DcnGeom gmax = g;
  gmax.B = std::min(bs, g.B);
  const DcnBwdHPlan pmax = dcn_bwd_h_plan(gmax);
  Carver c(ws, ws_bytes);
  u16* colg; float* partial; int* cursor; DcnEntries entries; void* sws;
  dcn_bwd_h_carve(c, gmax, pmax, &colg, &cursor, &entries, &sws, &partial);
  const long long om_bytes = om16 ? 2 : 4;
  const int cpg = g.Cin / g.dg, segs = K * g.dg;
  for (int s0 = 0; s0 < g.B; s0 += bs) {
    DcnGeom gc = g;
    gc.B = std::min(bs, g.B - s0);
    const DcnBwdHPlan p = dcn_bwd_h_plan(gc);
    FV2P_REQUIRE(p.splits <= pmax.splits_cap && p.npix <= pmax.npix && p.nkeys <= pmax.nkeys, FV2P_EWORKSPACE,
                 "dcn_backward_h: chunk of %d samples does not fit the workspace carved for %d", gc.B, gmax.B);
    const long long cpix = gc.B * pix;
    const u16* xc = x_nhwc + static_cast<long long>(s0) * g.H * g.W * g.Cin;
    const void* oc = static_cast<const char*>(offset) + static_cast<long long>(s0) * g.dg * 2 * K * pix * om_bytes;
    const void* mc = static_cast<const char*>(mask) + static_cast<long long>(s0) * g.dg * K * pix * om_bytes;
    const u16* dyc = dy_nhwc + static_cast<long long>(s0) * pix * g.Cout;
    u16* dxc = dx_nhwc + static_cast<long long>(s0) * g.H * g.W * g.Cin;
    void* doc = static_cast<char*>(doffset) + static_cast<long long>(s0) * g.dg * 2 * K * pix * om_bytes;
    void* dmc = static_cast<char*>(dmask) + static_cast<long long>(s0) * g.dg * K * pix * om_bytes;
    // 1. per-target sample lists (dcn.hip's kernels; lh / lw are the fp32 fractions the column pass forms)
    if (int rc = dcn_sample_lists(gc, oc, om16 ? T::code : 0, cursor, entries, sws, stream)) return rc;
    // 2. column gradients, grad_mask, grad_offset; small maps share a tile's segments among workgroups (dcn_backward_run's rule)
    int seg_split = 1;
    for (int sp = 1; sp <= segs; ++sp)
      if (segs % sp == 0) { seg_split = sp; if (ceil_div(cpix, 64) * sp >= 6 * dcn_cu_count()) break; }
    const int jb = static_cast<int>(ceil_div(g.Cout, 32));
#define DCN_CH(JB) dcn_col_h_launch<T, JB>(gc, xc, wt, oc, mc, om16, dyc, colg, doc, dmc, cpix, seg_split, stream)
    if (jb <= 1) DCN_CH(1); else if (jb <= 2) DCN_CH(2); else if (jb <= 4) DCN_CH(4); else DCN_CH(8);
#undef DCN_CH
    // 3. grad_input: the widest piece per lane that still fills the wave's lanes (development: FV2P_DCN_COL2IM_VEC = 1, 2, 4 or 8)
    int vec = cpg > 256 ? 8 : cpg > 128 ? 4 : cpg > 64 ? 2 : 1;
    if (const char* force = FV2P_DEV_ENV("FV2P_DCN_COL2IM_VEC")) {
      const int f = atoi(force);
      if (f == 1 || f == 2 || f == 4 || f == 8) vec = f;   // cpg % 16 == 0: every width divides it
    }
    if (vec == 8) dcn_col2im_h_launch<T, 8>(gc, colg, cursor, entries, dxc, stream);
    else if (vec == 4) dcn_col2im_h_launch<T, 4>(gc, colg, cursor, entries, dxc, stream);
    else if (vec == 2) dcn_col2im_h_launch<T, 2>(gc, colg, cursor, entries, dxc, stream);
    else dcn_col2im_h_launch<T, 1>(gc, colg, cursor, entries, dxc, stream);
    // 4. weight gradient: the chunk's pixel splits, added to dwt in ascending chunk order
    const int zt = p.ci_tiles * p.co_tiles;
    hipLaunchKernelGGL((dcn_bwd_weight_h_k<T>), dim3(static_cast<unsigned>(static_cast<long long>(p.splits) * K * zt)), dim3(256), 0, stream, gc, xc,
                       oc, mc, om16, dyc, p.pix_per_block, zt, partial);
    dcn_reduce_launch(partial, p.splits, static_cast<long long>(K) * g.Cin * g.Cout, dwt, s0 > 0, stream);
  }
  FV2P_LAUNCH_CHECK();
  return 0;
}

}  // namespace fv2p
using namespace fv2p;

extern "C" int fv2p_dcn_backward_h_supported(int c_in, int c_out, int deformable_group) {
  return fv2p_dcn_forward_h_supported(c_in, c_out, deformable_group) && c_out <= 256 && c_out % 8 == 0;
}

extern "C" size_t fv2p_dcn_backward_h_ws_bytes(int batch, int height, int width, int h_out, int w_out, int c_in, int c_out, int kh, int kw,
                                               int deformable_group) {
  return dcn_backward_h_ws({batch, height, width, c_in, c_out, h_out, w_out, kh, kw, 1, 1, 0, 0, 1, 1, deformable_group > 0 ? deformable_group : 1, 1});
}

extern "C" int fv2p_dcn_backward_h(const void* x_nhwc, const void* wt, const void* offset, const void* mask, const void* dy_nhwc,
                                   int batch, int height, int width, int c_in, int c_out, int h_out, int w_out, int kh, int kw,
                                   int sh, int sw, int ph, int pw, int dh, int dw, int deformable_group,
                                   void* dx_nhwc, void* doffset, void* dmask, float* dwt, void* ws, size_t ws_bytes, int dtype, int om_dtype,
                                   fv2p_stream_t stream_) {
  FV2P_DT16_OK("dcn_backward_h", dtype);
  FV2P_REQUIRE(om_dtype == 0 || om_dtype == dtype, FV2P_EINVAL, "dcn_backward_h: offset / mask dtype %d is neither fp32 (0) nor the call's dtype %d",
               om_dtype, dtype);
  const DcnGeom g = {batch, height, width, c_in, c_out, h_out, w_out, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group, 1};
  FV2P_REQUIRE(g.B >= 0 && g.H >= 1 && g.W >= 1 && g.Cin >= 1 && g.Cout >= 1 && g.kh >= 1 && g.kw >= 1 && g.sh >= 1 && g.sw >= 1 &&
                   g.dh >= 1 && g.dw >= 1 && g.dg >= 1 && g.Ho >= 1 && g.Wo >= 1,
               FV2P_EINVAL, "dcn_backward_h: bad geometry");
  FV2P_REQUIRE(fv2p_dcn_backward_h_supported(c_in, c_out, deformable_group), FV2P_ELIMIT,
               "dcn_backward_h: channels per deformable group (%d/%d) must be a multiple of 16, output channels (%d) a multiple of 8 up to 256",
               c_in, deformable_group, c_out);
  const hipStream_t stream = static_cast<hipStream_t>(stream_);
  const u16 *x = static_cast<const u16*>(x_nhwc), *w = static_cast<const u16*>(wt), *dy = static_cast<const u16*>(dy_nhwc);
  u16* dx = static_cast<u16*>(dx_nhwc);
  if (dtype == FV2P_DT_F16) return dcn_backward_h_run<BwdH16>(g, x, w, offset, mask, dy, dx, doffset, dmask, dwt, ws, ws_bytes, om_dtype != 0, stream);
  return dcn_backward_h_run<BwdB16>(g, x, w, offset, mask, dy, dx, doffset, dmask, dwt, ws, ws_bytes, om_dtype != 0, stream);
}
