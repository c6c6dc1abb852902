"""Cases of the 16-bit deformable-convolution forward (csrc/dcn_h.hip) with their results from oracle/dcn_oracle.py in float64.  Host only.

Exact cases: x and w in {-1, 0, 1} (x non-zero with probability 3/8), bias in {-2 .. 2}, and two families of sampling positions:
  integer     offsets in {-3 .. 3},       mask in {0, 1};
  half-pixel  offsets in 0.5 {-5 .. 5},   mask in {0, 0.5, 1}.
Every bilinear weight, column value and partial sum is then a multiple of 1/8 that fp32 holds exactly, so the kernel's fp32 sums are
exact in any order, and the result is exact in 16 bits (8 significant bits in bfloat16) when 8 max|ref| <= 256 (half-pixel) or
max|ref| <= 256 (integer): exact_case asserts it.

Random cases: x, w, bias and sigmoid masks rounded to the dtype first; offsets round(1.5 randn 64) / 64 clamped to |offset| < 4 -
representable in both formats, and base + offset is exact in fp32, so the bilinear weights are exact and nothing positional enters
the bound.  ref = the oracle on the rounded values in float64; S = the oracle on |x|, |w|, |bias| with the same offsets and masks."""
import functools

import torch

from oracle import dcn_oracle

# (Cin, Cout, deformable groups, (H, W), stride, dilation); B = 2, 3 x 3 taps, padding = dilation
GEOMETRIES = [
    (32, 48, 1, (11, 13), 1, 1),
    (64, 64, 2, (11, 13), 1, 2),
    (128, 200, 4, (9, 10), 1, 1),
    (64, 20, 1, (12, 9), 2, 1),
    (48, 16, 3, (7, 9), 1, 1),      # 16-channel deformable groups
    (256, 256, 4, (9, 8), 1, 1),
]
FAMILIES = ["integer", "half"]
# the (256, 256, 4) case is in the integer family only: its half-pixel results leave the exact range of bfloat16
EXACT = [(f, g) for f in FAMILIES for g in GEOMETRIES if not (f == "half" and g[0] == 256)]
BATCH, KSIZE = 2, 3
# seed of an exact case: 100 Cin + Cout, except where that draw leaves the exact range (half-pixel (128, 200): 8 max|ref| = 285 > 256);
# there the first later seed 100 Cin + Cout + 1000003 t that stays inside is taken.  A condition on the inputs, asserted in exact_case.
RESEED = {("half", 128, 200): 1}
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def geom_id(g):
    cin, cout, dg, (h, w), stride, dil = g
    return f"{cin}-{cout}-dg{dg}-{h}x{w}-s{stride}-d{dil}"


def out_size(g):
    _, _, _, (h, w), stride, dil = g
    pad = dil
    span = dil * (KSIZE - 1) + 1
    return (h + 2 * pad - span) // stride + 1, (w + 2 * pad - span) // stride + 1


def abi_geometry(g):
    """The 16 geometry integers of the C ABI."""
    cin, cout, dg, (h, w), stride, dil = g
    ho, wo = out_size(g)
    return (BATCH, h, w, cin, cout, ho, wo, KSIZE, KSIZE, stride, stride, dil, dil, dil, dil, dg)


def _oracle(x, offset, mask, w, bias, g):
    _, _, dg, _, stride, dil = g
    return dcn_oracle.modulated_deform_conv(x.double(), offset.double(), mask.double(), w.double(), bias.double(), (stride, stride), (dil, dil),
                                            (dil, dil), dg)


def _choice(gen, values, shape):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=gen)]


def _operands(gen, g):
    cin, cout, _, (h, w_), _, _ = g
    x = _choice(gen, [-1.0, 1.0], (BATCH, cin, h, w_)) * (torch.rand((BATCH, cin, h, w_), generator=gen) < 0.375).float()
    w = _choice(gen, [-1.0, 0.0, 1.0], (cout, cin, KSIZE, KSIZE))
    bias = _choice(gen, [-2.0, -1.0, 0.0, 1.0, 2.0], (cout,))
    return x, w, bias


@functools.lru_cache(maxsize=None)
def exact_case(family, g):
    """-> dict(x, w, bias, offset, mask, ref) of float32 host tensors whose values every format holds; ref exact in 16 bits."""
    cin, cout, dg, (h, w_), stride, dil = g
    ho, wo = out_size(g)
    gen = torch.Generator().manual_seed(100 * cin + cout + 1000003 * RESEED.get((family, cin, cout), 0))
    K = KSIZE * KSIZE
    if family == "integer":
        x, w, bias = _operands(gen, g)
        offset = _choice(gen, [float(v) for v in range(-3, 4)], (BATCH, dg * 2 * K, ho, wo))
        mask = _choice(gen, [0.0, 1.0], (BATCH, dg * K, ho, wo))
        scale = 1.0
    else:
        offset = _choice(gen, [0.5 * v for v in range(-5, 6)], (BATCH, dg * 2 * K, ho, wo))
        mask = _choice(gen, [0.0, 0.5, 1.0], (BATCH, dg * K, ho, wo))
        x, w, bias = _operands(gen, g)
        scale = 8.0
    ref = _oracle(x, offset, mask, w, bias, g)
    top = float(ref.abs().max())
    assert scale * top <= 256.0, (family, g, top)                 # exact in bfloat16's 8 significant bits
    assert torch.equal(ref * 8.0, torch.round(ref * 8.0))         # a multiple of 1/8
    assert torch.equal(ref.float().double(), ref)
    return dict(x=x, w=w, bias=bias, offset=offset, mask=mask, ref=ref.float(), top=top)


@functools.lru_cache(maxsize=None)
def random_case(g, dtype):
    """-> dict(x, w, bias, offset, mask: float32 host tensors of values representable in `dtype`; ref, S: float64)."""
    cin, cout, dg, (h, w_), stride, dil = g
    ho, wo = out_size(g)
    gen = torch.Generator().manual_seed(7 + 100 * cin + cout)
    K = KSIZE * KSIZE
    r16 = lambda t: t.to(dtype).float()
    x = r16(torch.randn((BATCH, cin, h, w_), generator=gen))
    w = r16(torch.randn((cout, cin, KSIZE, KSIZE), generator=gen) * (cin * K) ** -0.5)
    bias = r16(torch.randn((cout,), generator=gen) * 0.5)
    offset = (torch.round(1.5 * torch.randn((BATCH, dg * 2 * K, ho, wo), generator=gen) * 64.0) / 64.0).clamp(-4.0 + 1.0 / 64, 4.0 - 1.0 / 64)
    assert torch.equal(r16(offset), offset)
    mask = r16(torch.sigmoid(torch.randn((BATCH, dg * K, ho, wo), generator=gen)))
    ref = _oracle(x, offset, mask, w, bias, g)
    S = _oracle(x.abs(), offset, mask, w.abs(), bias.abs(), g)
    return dict(x=x, w=w, bias=bias, offset=offset, mask=mask, ref=ref, S=S)


def bound(case, g, dtype):
    """|got - ref| <= u (|ref| + e) + e + 2^-24 with e = (u + (K Cin + 6) 2^-24) S: u S for the one rounding of each column operand
    (the weights are given in 16 bits and are exact), (K Cin + 6) 2^-24 S for fp32 accumulation of K Cin products in any order plus the
    few fp32 roundings of a column value (three fused multiply-adds, one product, the mask, the bias); u (|ref| + e) for the one
    rounding of the result; 2^-24 for float16 results in the subnormal range.  Nothing in it is measured."""
    u = UNIT[dtype]
    e = (u + (KSIZE * KSIZE * g[0] + 6) * 2.0 ** -24) * case["S"]
    return u * (case["ref"].abs() + e) + e + 2.0 ** -24
