"""GPU: the deformable-convolution backward on float16 / bfloat16 maps (csrc/dcn_bwd_h.hip, DCN.NATIVE_16BIT_BACKWARD) through the DCN
modules and the raw C ABI.  Cases, float64 gradients and bounds come from dcn_bwd_half_cases.py.

  1. exact cases, raw entry point and ModulatedDeformConv with the flag on, offsets / masks in the dtype and in fp32: grad_weight and
     grad_bias equal the oracle bit for bit in fp32, every 16-bit gradient equals ref.to(dtype);
  2. the same cases with fv2p_dcn_set_colg_cap forcing one sample per chunk: the same bits;
  3. random cases: every gradient within the derived bound (dcn_bwd_half_cases.bound) - the forward's geometries, a 48-channel group, and
     WIDE: the geometries at which the host picks the kernels' other instantiations;
  4. operands and workspace embedded in NaN, outputs in sentinels (Cin/dg = 16, 48 and WIDE): the bits of the plain call, surroundings
     untouched;
  5. routing: flag on = one fv2p_dcn_backward_h and no fp32 kernel or converting transpose, two runs identical, channels-last stays
     channels-last, fp32 master weights get the unrounded fp32 gradient, declined geometries and the flag off keep today's route and
     bits, Cout = 20 goes through the zero-padded columns, an empty batch works;
  6. DCNv1 = DCNv2 with a unit mask."""
import pytest
import torch

import dcn_bwd_half_cases as bcases
import dcn_half_cases as cases
import fv2p_native as nat
from pcdet.ops.DeformableConvolutionV2PyTorch import DCN
from pcdet.ops.DeformableConvolutionV2PyTorch.modules.modulated_deform_conv import ModulatedDeformConv

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
DT_CODE = {torch.float16: 1, torch.bfloat16: 2}
dtype_id = lambda d: str(d).replace("torch.", "")
case_id = lambda v: v if isinstance(v, str) else cases.geom_id(v)
K = bcases.K
# a deformable group of 48 channels: a full 32-channel step followed by the 16-channel one
G48 = (96, 24, 2, (6, 7), 1, 1)
G16 = cases.GEOMETRIES[4]
# the kernels' other instantiations.  dcn_col2im_h_k holds 2 / 4 / 8 channels per lane for Cin/dg above 64 / 128 / 256 (80, 144, 272:
# each with lanes past the group's end; 528: a second pass over the group, partial too), and the column pass holds four dy fragments,
# two LDS-DMA pieces per wave, for Cout in 72 .. 128 (72: a ragged last fragment)
WIDE = [(80, 72, 1, (6, 7), 1, 1), (144, 104, 1, (5, 6), 1, 1), (272, 16, 1, (5, 6), 1, 1), (528, 8, 1, (4, 5), 1, 1)]


@pytest.fixture
def native(monkeypatch):
    monkeypatch.setattr(DCN, "NATIVE_16BIT_BACKWARD", True)


def _dev(t, dtype, gpu):
    return t.to(gpu).to(dtype)


def _host(t):
    return t.detach().float().cpu()


def _conv(g):
    _, _, dg, _, stride, dil = g
    return (3, 3, stride, stride, dil, dil, dil, dil, 1, dg, 64)


def _module(case, g, dtype, gpu):
    cin, cout, dg, _, stride, dil = g
    m = ModulatedDeformConv(cin, cout, cases.KSIZE, stride, dil, dil, 1, dg, 64, bias=True).to(gpu)
    with torch.no_grad():
        m.weight.copy_(case["w"].to(gpu))
        m.bias.copy_(case["bias"].to(gpu))
    return m.to(dtype) if dtype is not None else m


def _embedded(t, pad, fill=float("nan")):
    """-> (slice holding t's values, the surrounding buffer): `pad` elements of `fill` on either side"""
    buf = torch.full((t.numel() + 2 * pad,), fill, dtype=t.dtype, device=t.device)
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def _raw(case, g, dtype, om, gpu, embed=0):
    """fv2p_dcn_backward_h -> dict(input [B,C,H,W], offset, mask, weight [Cout,Cin,3,3] fp32) on the device; the output columns are
    zero-padded to a multiple of 8 as the caller must.  embed > 0: operands and workspace inside NaN, outputs inside sentinels (checked)."""
    geom = cases.abi_geometry(g)
    B, H, W, cin, cout, ho, wo = geom[:7]
    pad = (-cout) % 8
    geom = geom[:4] + (cout + pad,) + geom[5:]
    omt = dtype if om else torch.float32
    x = _dev(case["x"], dtype, gpu).permute(0, 2, 3, 1).contiguous()
    wt = torch.nn.functional.pad(_dev(case["w"], dtype, gpu).permute(2, 3, 1, 0).reshape(K, cin, cout), (0, pad)).contiguous()
    dy = torch.nn.functional.pad(_dev(case["dy"], dtype, gpu).permute(0, 2, 3, 1), (0, pad)).contiguous()
    off, msk = _dev(case["offset"], omt, gpu).contiguous(), _dev(case["mask"], omt, gpu).contiguous()
    dx = torch.zeros((B, H, W, cin), dtype=dtype, device=gpu)
    doff, dmask = torch.zeros_like(off), torch.zeros_like(msk)
    dwt = torch.zeros((K, cin, cout + pad), dtype=torch.float32, device=gpu)
    nb = nat.lib().fv2p_dcn_backward_h_ws_bytes(B, H, W, ho, wo, cin, cout + pad, 3, 3, g[2])
    if embed:
        (x, _), (wt, _), (dy, _), (off, _), (msk, _) = (_embedded(t, embed) for t in (x, wt, dy, off, msk))
        outs = [_embedded(t, embed, fill=7.0) for t in (dx, doff, dmask, dwt)]
        dx, doff, dmask, dwt = (v for v, _ in outs)
        ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=gpu)   # every 16-bit and fp32 word of it a NaN
    else:
        ws = nat.workspace(nb, x.device)
    nat.call("fv2p_dcn_backward_h", x, wt, off, msk, dy, *geom, dx, doff, dmask, dwt, ws, ws.numel(), DT_CODE[dtype], DT_CODE[dtype] if om else 0,
             nat.stream())
    torch.cuda.synchronize()
    if embed:
        for v, buf in outs:
            assert bool((buf[:embed] == 7.0).all()) and bool((buf[embed + v.numel():] == 7.0).all())
    return dict(input=dx.permute(0, 3, 1, 2), offset=doff, mask=dmask,
                weight=dwt[:, :, :cout].reshape(3, 3, cin, cout).permute(3, 2, 0, 1).contiguous())


def _check_exact(got, ref, dtype, omt, wdtype, where):
    want = {"input": dtype, "offset": omt, "mask": omt, "weight": wdtype, "bias": wdtype}
    for name, t in got.items():
        assert t.dtype == want[name], (where, name, t.dtype)
        assert torch.equal(t.detach().cpu(), ref[name].to(want[name])), (where, name)


@pytest.mark.parametrize("family,g", cases.EXACT, ids=case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_exact_cases_through_the_raw_entry_point_equal_the_oracle_bit_for_bit(gpu, dtype, family, g):
    case = bcases.exact_case(family, g)
    for om in (0, 1):
        _check_exact(_raw(case, g, dtype, om, gpu), case["ref"], dtype, dtype if om else torch.float32, torch.float32, f"om {om}")


@pytest.mark.parametrize("family,g", cases.EXACT, ids=case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_exact_cases_through_the_module_equal_the_oracle_bit_for_bit(gpu, native, dtype, family, g):
    case = bcases.exact_case(family, g)
    m = _module(case, g, dtype, gpu)
    dy = _dev(case["dy"], dtype, gpu)
    for omt in (dtype, torch.float32):
        x, off, msk = _dev(case["x"], dtype, gpu).requires_grad_(True), _dev(case["offset"], omt, gpu).requires_grad_(True), _dev(case["mask"], omt, gpu).requires_grad_(True)
        m.zero_grad(set_to_none=True)
        m(x, off, msk).backward(dy)
        got = dict(input=x.grad, offset=off.grad, mask=msk.grad, weight=m.weight.grad, bias=m.bias.grad)
        _check_exact(got, case["ref"], dtype, omt, dtype, omt)
        assert x.grad.is_contiguous()


@pytest.mark.parametrize("family,g", cases.EXACT, ids=case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_one_sample_per_chunk_gives_the_same_bits(gpu, dtype, family, g):
    case = bcases.exact_case(family, g)
    ho, wo = cases.out_size(g)
    whole = _raw(case, g, dtype, 1, gpu)
    try:
        nat.call("fv2p_dcn_set_colg_cap", ho * wo * K * g[0] * 4)   # the column gradients of ONE sample
        chunked = _raw(case, g, dtype, 1, gpu)
    finally:
        nat.call("fv2p_dcn_set_colg_cap", 0)
    _check_exact(chunked, case["ref"], dtype, dtype, torch.float32, "chunked")
    for name in whole:
        assert torch.equal(whole[name], chunked[name]), name


@pytest.mark.parametrize("g", cases.GEOMETRIES + [G48] + WIDE, ids=case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_random_cases_stay_within_the_derived_bound(gpu, native, dtype, g):
    case = bcases.random_case(g, dtype)
    m = _module(case, g, dtype, gpu)
    x, off, msk = (_dev(case[k], dtype, gpu).requires_grad_(True) for k in ("x", "offset", "mask"))
    m(x, off, msk).backward(_dev(case["dy"], dtype, gpu))
    runs = {
        "module": (dict(input=x.grad, offset=off.grad, mask=msk.grad, weight=m.weight.grad, bias=m.bias.grad), {n: dtype for n in bcases.NAMES}),
        "raw fp32 offsets": (_raw(case, g, dtype, 0, gpu), dict(input=dtype, offset=torch.float32, mask=torch.float32, weight=torch.float32)),
        "raw 16-bit offsets": (_raw(case, g, dtype, 1, gpu), dict(input=dtype, offset=dtype, mask=dtype, weight=torch.float32)),
    }
    worst = 0.0
    for where, (got, formats) in runs.items():
        lim = bcases.bound(case, g, dtype, {**{n: dtype for n in bcases.NAMES}, **formats})
        for name, t in got.items():
            assert t.dtype == formats[name], (where, name)
            ratio = float(((_host(t).double() - case["ref"][name]).abs() / lim[name]).max())
            worst = max(worst, ratio)
            print(f"dcn16bwd {dtype_id(dtype)} {cases.geom_id(g)} {where} grad_{name}: largest |got - ref| / bound = {ratio:.3f}")
            assert ratio <= 1.0, (where, name, ratio)
    assert torch.equal(runs["module"][0]["input"], runs["raw 16-bit offsets"][0]["input"])
    assert torch.equal(runs["module"][0]["offset"], runs["raw 16-bit offsets"][0]["offset"])
    assert worst > 0.0   # a 16-bit result of random operands is not the float64 one


@pytest.mark.parametrize("g", [G16, G48] + WIDE, ids=case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_operands_embedded_in_nan_give_the_same_bits_and_leave_the_surroundings_alone(gpu, dtype, g):
    case = bcases.random_case(g, dtype)
    for om in (0, 1):
        tight, inside = _raw(case, g, dtype, om, gpu), _raw(case, g, dtype, om, gpu, embed=64)
        for name in tight:
            assert not torch.isnan(inside[name].float()).any(), name
            assert torch.equal(tight[name], inside[name]), name


class _Recorder:
    def __init__(self):
        self.names, self.inner = [], nat.call

    def __call__(self, name, *args):
        self.names.append(name)
        return self.inner(name, *args)


FP32_ROUTE = ("fv2p_dcn_backward", "fv2p_dcn_backward_grouped", "fv2p_transpose_batched_widen", "fv2p_transpose_batched_round", "fv2p_transpose_batched")


def _backward_names(monkeypatch, fn):
    rec = _Recorder()
    monkeypatch.setattr(nat, "call", rec)
    try:
        out = fn()
    finally:
        monkeypatch.setattr(nat, "call", rec.inner)
    return out, rec.names


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_the_flag_routes_the_module_to_the_16_bit_entry_point(gpu, native, dtype, monkeypatch):
    g = cases.GEOMETRIES[1]
    case = bcases.random_case(g, dtype)
    dy = _dev(case["dy"], dtype, gpu)

    def run(m, x, autocast=False):
        x = x.detach().requires_grad_(True)
        off, msk = (_dev(case[k], dtype, gpu).requires_grad_(True) for k in ("offset", "mask"))
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=dtype, enabled=autocast):
            y = m(x, off, msk)
        _, names = _backward_names(monkeypatch, lambda: y.backward(dy if not _cl(y) else dy.contiguous(memory_format=torch.channels_last)))
        return dict(input=x.grad, offset=off.grad, mask=msk.grad, weight=m.weight.grad, bias=m.bias.grad), names

    _cl = lambda t: t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()
    m = _module(case, g, dtype, gpu)
    x = _dev(case["x"], dtype, gpu)
    first, names = run(m, x)
    assert names.count("fv2p_dcn_backward_h") == 1 and not any(n in names for n in FP32_ROUTE), names
    assert names.count("fv2p_transpose_batched_h") == 3, names   # x, grad_output in; grad_input out
    second, _ = run(m, x)
    for name in first:
        assert first[name].dtype == dtype and torch.equal(first[name], second[name]), name
    # channels-last in, channels-last grad_input out, no layout copy at all
    last, names = run(m, x.contiguous(memory_format=torch.channels_last))
    assert names == ["fv2p_dcn_backward_h"], names
    assert _cl(last["input"])
    for name in first:
        assert torch.equal(first[name], last[name]), name
    # fp32 master weights under autocast: the weight is rounded once on the way in, its gradient is the kernel's fp32 buffer
    plain = _module(case, g, None, gpu)
    with torch.no_grad():
        plain.weight.copy_(m.weight.float())
        plain.bias.copy_(m.bias.float())
    cast, names = run(plain, x, autocast=True)
    assert names.count("fv2p_dcn_backward_h") == 1 and not any(n in names for n in FP32_ROUTE), names
    raw = _raw(case, g, dtype, 1, gpu)
    assert cast["weight"].dtype == torch.float32 and torch.equal(cast["weight"], raw["weight"])
    assert not torch.equal(cast["weight"], cast["weight"].to(dtype).float())   # unrounded
    assert torch.equal(first["weight"], raw["weight"].to(dtype)) and torch.equal(cast["input"], first["input"])


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_declined_geometries_and_the_flag_off_keep_todays_route_and_bits(gpu, dtype, monkeypatch):
    gen = torch.Generator().manual_seed(21)

    def problem(cin, cout, dg, groups):
        B, H, W = 2, 7, 9
        r = lambda *s: torch.randn(s, generator=gen)
        x, w, b = r(B, cin, H, W), r(cout, cin // groups, 3, 3) * 0.1, r(cout)
        off, msk, dy = r(B, dg * 18, H, W) * 1.5, torch.rand((B, dg * 9, H, W), generator=gen), r(B, cout, H, W)
        return [t.to(gpu).to(dtype) for t in (x, w, b, off, msk, dy)], (3, 3, 1, 1, 1, 1, 1, 1, groups, dg, 64)

    for cin, cout, dg, groups in [(16, 24, 2, 1), (32, 32, 1, 2), (32, 264, 1, 1)]:   # 8 channels per deformable group; conv groups; Cout > 256
        args, conv = problem(cin, cout, dg, groups)
        monkeypatch.setattr(DCN, "NATIVE_16BIT_BACKWARD", True)
        got, names = _backward_names(monkeypatch, lambda: DCN.modulated_deform_conv_backward(*args, *conv))
        monkeypatch.setattr(DCN, "NATIVE_16BIT_BACKWARD", False)
        want = DCN.modulated_deform_conv_backward(*args, *conv)
        assert "fv2p_dcn_backward_h" not in names, names
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and torch.equal(a, b), (cin, cout, dg, groups)
    # a geometry the kernel takes, flag off: one fv2p_dcn_backward between two widening transposes and a rounding one, the fp32 bits
    args, conv = problem(64, 64, 2, 1)
    got, names = _backward_names(monkeypatch, lambda: DCN.modulated_deform_conv_backward(*args, *conv))
    assert names.count("fv2p_dcn_backward") == 1 and names.count("fv2p_transpose_batched_widen") == 2, names
    assert names.count("fv2p_transpose_batched_round") == 1 and "fv2p_dcn_backward_h" not in names, names
    want = DCN.modulated_deform_conv_backward(*(t.float() for t in args), *conv)
    assert got[0].dtype == dtype and torch.equal(got[0], want[0].to(dtype))
    for a, b in zip(got[1:], want[1:]):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    # fp32 tensors with the flag on: the fp32 route
    monkeypatch.setattr(DCN, "NATIVE_16BIT_BACKWARD", True)
    again, names = _backward_names(monkeypatch, lambda: DCN.modulated_deform_conv_backward(*(t.float() for t in args), *conv))
    assert "fv2p_dcn_backward_h" not in names and all(torch.equal(a, b) for a, b in zip(again, want)), names


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_padded_output_columns_and_an_empty_batch(gpu, native, dtype, monkeypatch):
    g = cases.GEOMETRIES[3]   # Cout = 20
    case = bcases.exact_case("half", g)
    args = [_dev(case[k], dtype, gpu) for k in ("x", "w", "bias", "offset", "mask", "dy")]
    got, names = _backward_names(monkeypatch, lambda: DCN.modulated_deform_conv_backward(*args, *_conv(g)))
    assert names.count("fv2p_dcn_backward_h") == 1 and not any(n in names for n in FP32_ROUTE), names
    assert tuple(got[3].shape) == tuple(case["w"].shape) and tuple(got[4].shape) == (20,)
    _check_exact(dict(zip(bcases.NAMES, got[:4])), case["ref"], dtype, dtype, dtype, "padded")
    assert got[4].dtype == torch.float32 and torch.equal(got[4].cpu(), case["ref"]["bias"].float())
    x, w, b, off, msk, dy = args
    empty = DCN.modulated_deform_conv_backward(x[:0], w, b, off[:0], msk[:0], dy[:0], *_conv(g))
    torch.cuda.synchronize()
    assert tuple(empty[0].shape) == (0,) + tuple(x.shape[1:]) and empty[0].dtype == dtype
    assert empty[1].numel() == 0 and empty[2].numel() == 0
    assert not empty[3].float().abs().any() and not empty[4].abs().any()


@pytest.mark.parametrize("g", [cases.GEOMETRIES[1], G16], ids=case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_dcnv1_backward_equals_dcnv2_with_a_unit_mask(gpu, native, dtype, g, monkeypatch):
    case = bcases.random_case(g, dtype)
    x, w, b, off, dy = (_dev(case[k], dtype, gpu) for k in ("x", "w", "bias", "offset", "dy"))
    v1, names = _backward_names(monkeypatch, lambda: DCN.deform_conv_backward(x, w, b, off, dy, *_conv(g)))
    assert names.count("fv2p_dcn_backward_h") == 1 and not any(n in names for n in FP32_ROUTE), names
    ones = torch.ones_like(_dev(case["mask"], dtype, gpu))
    v2 = DCN.modulated_deform_conv_backward(x, w, b, off, ones, dy, *_conv(g))
    assert len(v1) == 4
    for a, b_ in zip(v1, (v2[0], v2[1], v2[3], v2[4])):
        assert a.dtype == b_.dtype and torch.equal(a, b_)
