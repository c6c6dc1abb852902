"""Cases of the 16-bit deformable-convolution backward (csrc/dcn_bwd_h.hip): the operands of dcn_half_cases.py, a grad_output, and the
five gradients in float64 from autograd through oracle/dcn_oracle.py.  Host only.

Exact cases: the operands of dcn_half_cases.exact_case and grad_output in {-1, 0, 1}, non-zero with probability 1/8 (seed
9 + 100 Cin + Cout: the signs are drawn first, then the density mask).  exact_case asserts the conditions under which every
intermediate of the kernels is exact:
  dcol = sum_co w dy is an integer and colg = dcol * mask a multiple of 1/2 with 2 max|colg| <= 256: it survives its rounding to
  8 significant bits; the column operand of the weight gradient is a multiple of 1/8 of magnitude <= 1 (dcn_half_cases);
  all five float64 gradients are multiples of 1/16 that fp32 holds, so every fp32 partial sum is exact in any order.
grad_weight and grad_bias then equal the oracle bit for bit in fp32, and a 16-bit output equals ref.to(dtype): ONE rounding of the exact
fp32 value (the results themselves need not be representable).

Random cases: the operands of dcn_half_cases.random_case (representable in the dtype; base + offset exact in fp32, so every bilinear
weight and fraction is exact and nothing positional enters a bound) and grad_output = randn rounded to the dtype.  With u the unit
roundoff of the dtype, e = 2^-24 that of fp32, and the sums of absolute terms
  A[p,k,ci]  = sum_co |w| |dy|                                    (absolute column gradient)
  S_x, S_w, S_m = the oracle's gradients on |x|, |w|, |dy| (same offsets, masks >= 0): every term of those sums is non-negative
  S_o        = the host restatement below: m (c_0 A_0 + c_1 A_1 + c_2 A_2 + c_3 A_3) with A_q = sum_ci A |x at corner q| and the ABSOLUTE
               corner coefficients c_q (the signed ones cancel under autograd, which would under-state the sum)
the kernels' errors before the output rounding are bounded by
  grad_input   e_x = ((1 + u) (u + (Cout + 2) e) + n_s e) S_x + n_s 2^-25 : dcol's fp32 accumulation over Cout exact products, the
               product with the mask, ONE rounding of colg to the dtype (2^-25 each where it falls into float16's subnormals), and the
               fp32 sum of at most n_s = K Ho Wo samples per input pixel and deformable group;
  grad_weight  e_w = (u + (npix + 6) e) S_w : ONE rounding of the column operand and the few fp32 roundings that form it
               (dcn_half_cases.bound), fp32 accumulation over the npix = B Ho Wo pixels in any order;
  grad_mask    e_m = (Cout + cpg + 8) e S_m : dcol's accumulation, the fmaf chain over the cpg channels of the group and the two
               cross-lane adds, four products and three adds - no 16-bit rounding enters;
  grad_offset  e_o = (Cout + cpg + 10) e S_o : the same, and the product with the mask;
  grad_bias    e_b = npix e sum_p |dy| : an fp32 sum.
and |got - ref| <= u_out (|ref| + e) + e + 2^-24, u_out the unit roundoff of the OUTPUT's format (2^-24 for the fp32 outputs; 2^-24
absolute for float16 results in the subnormal range).  Nothing in it is measured."""
import functools

import torch

import dcn_half_cases as cases
from oracle import dcn_oracle

NAMES = ("input", "offset", "mask", "weight", "bias")
E32 = 2.0 ** -24
K = cases.KSIZE * cases.KSIZE


def _conv_args(g):
    _, _, dg, _, stride, dil = g
    return (stride, stride), (dil, dil), (dil, dil), dg


def gradients(x, offset, mask, w, bias, dy, g):
    """float64 gradients (input, offset, mask, weight, bias) of <oracle(...), dy> by autograd"""
    leaves = [t.double().clone().requires_grad_(True) for t in (x, offset, mask, w, bias)]
    y = dcn_oracle.modulated_deform_conv(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], *_conv_args(g))
    y.backward(dy.double())
    return {n: t.grad for n, t in zip(NAMES, leaves)}


def _dcol(w, dy):
    """[B, K, Cin, Ho, Wo] = sum_co w[co, ci, k] dy[b, co, ho, wo]"""
    cout, cin = w.shape[:2]
    return torch.einsum("ock,bohw->bkchw", w.double().reshape(cout, cin, K), dy.double())


def exact_dy(g):
    cin, cout = g[0], g[1]
    ho, wo = cases.out_size(g)
    gen = torch.Generator().manual_seed(9 + 100 * cin + cout)
    shape = (cases.BATCH, cout, ho, wo)
    signs = cases._choice(gen, [-1.0, 1.0], shape)
    return signs * (torch.rand(shape, generator=gen) < 0.125).float()


@functools.lru_cache(maxsize=None)
def exact_case(family, g):
    """-> dict(x, w, bias, offset, mask, dy: float32 host tensors every format holds; ref: the five float64 gradients)"""
    case = dict(cases.exact_case(family, g))
    cin, _, dg, _, _, _ = g
    dy = exact_dy(g)
    dcol = _dcol(case["w"], dy)
    colg = dcol * case["mask"].double().view(cases.BATCH, dg, K, *dy.shape[2:]).permute(0, 2, 1, 3, 4).repeat_interleave(cin // dg, dim=2)
    assert torch.equal(colg * 2.0, torch.round(colg * 2.0)), (family, g)
    assert 2.0 * float(colg.abs().max()) <= 256.0, (family, g, float(colg.abs().max()))
    ref = gradients(case["x"], case["offset"], case["mask"], case["w"], case["bias"], dy, g)
    for name, t in ref.items():
        assert torch.equal(t * 16.0, torch.round(t * 16.0)), (family, g, name)
        assert torch.equal(t.float().double(), t), (family, g, name)
    case.update(dy=dy, ref=ref, top=max(float(t.abs().max()) for t in ref.values()), dcol_top=float(dcol.abs().max()))
    return case


def offset_abs_sums(x, w, offset, mask, dy, g):
    """S_o [B, dg*2*K, Ho, Wo]: grad_offset's per-corner sums with absolute terms and absolute corner coefficients - the oracle's sampling
    (validity, floor, corners inside the map) restated on |x| and A = sum_co |w| |dy|.  Also returns S_m built the same way."""
    cin, _, dg, (H, W), stride, dil = g
    B, cpg = x.shape[0], cin // dg
    ho_n, wo_n = cases.out_size(g)
    A = _dcol(w.abs(), dy.abs())
    xa, offset, mask = x.double().abs(), offset.double(), mask.double()
    ho = torch.arange(ho_n, dtype=torch.float64).view(1, ho_n, 1)
    wo = torch.arange(wo_n, dtype=torch.float64).view(1, 1, wo_n)
    s_o, s_m = torch.zeros_like(offset), torch.zeros_like(mask)
    for d in range(dg):
        xg = xa[:, d * cpg:(d + 1) * cpg].reshape(B, cpg, H * W)
        for k in range(K):
            i, j = k // cases.KSIZE, k % cases.KSIZE
            h_im = ho * stride - dil + i * dil + offset[:, d * 2 * K + 2 * k]
            w_im = wo * stride - dil + j * dil + offset[:, d * 2 * K + 2 * k + 1]
            valid = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
            h_low, w_low = torch.floor(h_im), torch.floor(w_im)
            lh, lw = h_im - h_low, w_im - w_low
            hh, hw = 1 - lh, 1 - lw
            m = mask[:, d * K + k]
            sh = sw = sm = 0
            for hq, wq, wt, ch, cw in ((h_low, w_low, hh * hw, hw, hh), (h_low, w_low + 1, hh * lw, lw, hh), (h_low + 1, w_low, lh * hw, hw, lh),
                                       (h_low + 1, w_low + 1, lh * lw, lw, lh)):
                ok = (valid & (hq >= 0) & (hq <= H - 1) & (wq >= 0) & (wq <= W - 1)).double()
                idx = (hq.clamp(0, H - 1) * W + wq.clamp(0, W - 1)).long().view(B, 1, -1).expand(B, cpg, ho_n * wo_n)
                v = torch.gather(xg, 2, idx).view(B, cpg, ho_n, wo_n)
                a_q = (A[:, k, d * cpg:(d + 1) * cpg] * v).sum(1) * ok
                sh, sw, sm = sh + ch * a_q, sw + cw * a_q, sm + wt * a_q
            s_o[:, d * 2 * K + 2 * k], s_o[:, d * 2 * K + 2 * k + 1], s_m[:, d * K + k] = m * sh, m * sw, sm
    return s_o, s_m


@functools.lru_cache(maxsize=None)
def random_case(g, dtype):
    """-> dict(x, w, bias, offset, mask, dy: float32 host tensors of values representable in `dtype`; ref, S: dicts of float64)"""
    case = dict(cases.random_case(g, dtype))
    cin, cout = g[0], g[1]
    ho, wo = cases.out_size(g)
    gen = torch.Generator().manual_seed(11 + 100 * cin + cout)
    dy = torch.randn((cases.BATCH, cout, ho, wo), generator=gen).to(dtype).float()
    ref = gradients(case["x"], case["offset"], case["mask"], case["w"], case["bias"], dy, g)
    S = gradients(case["x"].abs(), case["offset"], case["mask"], case["w"].abs(), case["bias"].abs(), dy.abs(), g)
    S["offset"], s_m = offset_abs_sums(case["x"], case["w"], case["offset"], case["mask"], dy, g)
    # the restatement sums what autograd sums where every term is non-negative
    assert torch.allclose(s_m, S["mask"], rtol=1e-12, atol=1e-12)
    assert bool((S["offset"] + 1e-12 >= ref["offset"].abs()).all())
    case.update(dy=dy, ref=ref, S=S)
    return case


def error_before_rounding(case, g, dtype):
    """e per gradient (the module docstring)"""
    cin, cout, dg = g[0], g[1], g[2]
    ho, wo = cases.out_size(g)
    u, S = cases.UNIT[dtype], case["S"]
    npix, n_s, cpg = cases.BATCH * ho * wo, K * ho * wo, cin // dg
    return {
        "input": ((1.0 + u) * (u + (cout + 2) * E32) + n_s * E32) * S["input"] + n_s * 2.0 ** -25,
        "weight": (u + (npix + 6) * E32) * S["weight"],
        "mask": (cout + cpg + 8) * E32 * S["mask"],
        "offset": (cout + cpg + 10) * E32 * S["offset"],
        "bias": npix * E32 * S["bias"],
    }


def bound(case, g, dtype, out_dtypes):
    """|got - ref| <= u_out (|ref| + e) + e + 2^-24 per gradient; out_dtypes: name -> the format the gradient arrives in"""
    e = error_before_rounding(case, g, dtype)
    unit = lambda d: E32 if d == torch.float32 else cases.UNIT[d]
    return {n: unit(out_dtypes[n]) * (case["ref"][n].abs() + e[n]) + e[n] + E32 for n in NAMES}
