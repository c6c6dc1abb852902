"""GPU: the deformable-convolution forward on float16 / bfloat16 maps (csrc/dcn_h.hip) through the DCN modules and the raw C ABI.
Cases and oracle results come from dcn_half_cases.py.

  1. exact cases: module (contiguous and channels-last input, offsets / masks in the dtype and in fp32, DCNv1 with its all-ones mask)
     and raw entry point (om_dtype 0 and dtype) equal the oracle bit for bit;
  2. random cases: |got - ref| <= u (|ref| + e) + e + 2^-24 element-wise, e = (u + (K Cin + 6) 2^-24) S (dcn_half_cases.bound);
  3. operands embedded in NaN: same bits as from tight buffers, y's surroundings untouched (no out-of-range read hidden by a zero operand);
  4. no fp32 copy of a map: the peak memory of a forward stays below the size of the fp32 copies of x and y alone;
  5. two runs identical; .half() / .bfloat16() and autocast modules return the dtype through fv2p_dcn_forward_h; empty batch;
  6. geometries the kernel declines, fp32 calls and NATIVE_16BIT = False keep the earlier route and its bits;
  7. the backward after a native forward: all five gradients are the fp32 backward's, cast; the two conversion transposes equal their
     two-step forms on ragged sizes."""
import pytest
import torch

import dcn_half_cases as cases
import fv2p_native as nat
from oracle import dcn_oracle
from pcdet.ops.DeformableConvolutionV2PyTorch import DCN
from pcdet.ops.DeformableConvolutionV2PyTorch.modules.deform_conv import DeformConv
from pcdet.ops.DeformableConvolutionV2PyTorch.modules.modulated_deform_conv import ModulatedDeformConv

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
DT_CODE = {torch.float16: 1, torch.bfloat16: 2}
dtype_id = lambda d: str(d).replace("torch.", "")
case_id = lambda v: v if isinstance(v, str) else cases.geom_id(v)
# a deformable group of 48 channels: a full 32-channel step followed by the 16-channel one
G48 = (96, 24, 2, (6, 7), 1, 1)
RANDOM = cases.GEOMETRIES + [G48]


def _dev(t, dtype, gpu):
    return t.to(gpu).to(dtype)


def _host(t):
    return t.detach().float().cpu()


def _module(case, g, dtype, gpu, v1=False):
    cin, cout, dg, _, stride, dil = g
    cls = DeformConv if v1 else ModulatedDeformConv
    m = cls(cin, cout, cases.KSIZE, stride, dil, dil, 1, dg, 64, bias=not v1).to(gpu)
    with torch.no_grad():
        m.weight.copy_(case["w"].to(gpu))
        m.bias.copy_(case["bias"].to(gpu) if not v1 else torch.zeros(cout))
    return m.to(dtype) if dtype is not None else m


def _raw(case, g, dtype, om, gpu):
    """fv2p_dcn_forward_h on tight buffers -> y [B, Cout, Ho, Wo] on the device"""
    geom = cases.abi_geometry(g)
    B, H, W, cin, cout, ho, wo = geom[:7]
    x = _dev(case["x"], dtype, gpu).permute(0, 2, 3, 1).contiguous()
    wt_oc = _dev(case["w"], dtype, gpu).permute(2, 3, 0, 1).reshape(cases.KSIZE ** 2, cout, cin).contiguous()
    omt = dtype if om else torch.float32
    off, msk = _dev(case["offset"], omt, gpu).contiguous(), _dev(case["mask"], omt, gpu).contiguous()
    y = torch.empty((B, ho, wo, cout), dtype=dtype, device=gpu)
    nat.call("fv2p_dcn_forward_h", x, wt_oc, case["bias"].to(gpu), off, msk, *geom, y, DT_CODE[dtype], DT_CODE[dtype] if om else 0, nat.stream())
    torch.cuda.synchronize()
    return y.permute(0, 3, 1, 2)


@pytest.mark.parametrize("family,g", cases.EXACT, ids=case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_exact_cases_through_the_raw_entry_point_equal_the_oracle_bit_for_bit(gpu, dtype, family, g):
    case = cases.exact_case(family, g)
    for om in (0, 1):
        assert torch.equal(_host(_raw(case, g, dtype, om, gpu)), case["ref"]), f"om_dtype {'dtype' if om else 'fp32'}"


@pytest.mark.parametrize("family,g", cases.EXACT, ids=case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_exact_cases_through_the_module_equal_the_oracle_bit_for_bit(gpu, dtype, family, g):
    case = cases.exact_case(family, g)
    m = _module(case, g, dtype, gpu)
    x = _dev(case["x"], dtype, gpu)
    with torch.no_grad():
        for omt in (dtype, torch.float32):
            off, msk = _dev(case["offset"], omt, gpu), _dev(case["mask"], omt, gpu)
            y = m(x, off, msk)
            assert y.dtype == dtype and y.is_contiguous() and torch.equal(_host(y), case["ref"]), omt
        y = m(x.contiguous(memory_format=torch.channels_last), off, msk)
        assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last) and torch.equal(_host(y), case["ref"]), "channels-last"


@pytest.mark.parametrize("g", cases.GEOMETRIES, ids=case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_dcnv1_integer_cases_equal_the_oracle_bit_for_bit(gpu, dtype, g):
    case = cases.exact_case("integer", g)
    _, _, dg, _, stride, dil = g
    ref = dcn_oracle.modulated_deform_conv(case["x"].double(), case["offset"].double(), torch.ones_like(case["mask"]).double(), case["w"].double(),
                                           None, (stride, stride), (dil, dil), (dil, dil), dg)
    assert float(ref.abs().max()) <= 256.0   # integers that both formats hold
    m = _module(case, g, dtype, gpu, v1=True)
    with torch.no_grad():
        y = m(_dev(case["x"], dtype, gpu), _dev(case["offset"], dtype, gpu))
    assert y.dtype == dtype and torch.equal(_host(y).double(), ref)


@pytest.mark.parametrize("g", RANDOM, ids=case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_random_cases_stay_within_the_derived_bound(gpu, dtype, g):
    case = cases.random_case(g, dtype)
    lim = cases.bound(case, g, dtype)
    m = _module(case, g, dtype, gpu)
    with torch.no_grad():
        ym = m(_dev(case["x"], dtype, gpu), _dev(case["offset"], dtype, gpu), _dev(case["mask"], dtype, gpu))
    worst = 0.0
    got = {"module": ym, "raw fp32 offsets": _raw(case, g, dtype, 0, gpu), "raw 16-bit offsets": _raw(case, g, dtype, 1, gpu)}
    for name, y in got.items():
        assert y.dtype == dtype
        ratio = float(((_host(y).double() - case["ref"]).abs() / lim).max())
        worst = max(worst, ratio)
        print(f"dcn16 {dtype_id(dtype)} {cases.geom_id(g)} {name}: largest |got - ref| / bound = {ratio:.3f}")
        assert ratio <= 1.0, (name, ratio)
    assert torch.equal(got["module"], got["raw 16-bit offsets"]) and torch.equal(got["module"], got["raw fp32 offsets"])
    assert worst > 0.0   # a 16-bit result of random operands is not the float64 one


def _embedded(t, pad, fill=float("nan")):
    """-> (slice holding t's values, the surrounding buffer): `pad` elements of `fill` on either side"""
    buf = torch.full((t.numel() + 2 * pad,), fill, dtype=t.dtype, device=t.device)
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


@pytest.mark.parametrize("g", [cases.GEOMETRIES[4], G48, cases.GEOMETRIES[3], cases.GEOMETRIES[2]], ids=case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_operands_embedded_in_nan_give_the_same_bits_and_leave_the_surroundings_alone(gpu, dtype, g):
    case = cases.random_case(g, dtype)
    geom = cases.abi_geometry(g)
    B, H, W, cin, cout, ho, wo = geom[:7]
    for om in (0, 1):
        tight = _raw(case, g, dtype, om, gpu).permute(0, 2, 3, 1).contiguous()
        omt = dtype if om else torch.float32
        x, _ = _embedded(_dev(case["x"], dtype, gpu).permute(0, 2, 3, 1).contiguous(), 64)
        wt, _ = _embedded(_dev(case["w"], dtype, gpu).permute(2, 3, 0, 1).reshape(9, cout, cin).contiguous(), 64)
        off, _ = _embedded(_dev(case["offset"], omt, gpu).contiguous(), 64)
        msk, _ = _embedded(_dev(case["mask"], omt, gpu).contiguous(), 64)
        bias, _ = _embedded(case["bias"].to(gpu), 64)
        y, ybuf = _embedded(torch.zeros((B, ho, wo, cout), dtype=dtype, device=gpu), 64, fill=7.0)
        nat.call("fv2p_dcn_forward_h", x, wt, bias, off, msk, *geom, y, DT_CODE[dtype], DT_CODE[dtype] if om else 0, nat.stream())
        torch.cuda.synchronize()
        assert not torch.isnan(y.float()).any()
        assert torch.equal(y, tight)
        assert bool((ybuf[:64] == 7.0).all()) and bool((ybuf[64 + y.numel():] == 7.0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_the_forward_makes_no_fp32_copy_of_a_map(gpu, dtype):
    B, C, H, W = 2, 128, 48, 44
    gen = torch.Generator().manual_seed(3)
    m = ModulatedDeformConv(C, C, 3, 1, 1, 1, 1, 1, 64, bias=True).to(gpu).to(dtype)
    x = torch.randn((B, C, H, W), generator=gen).to(gpu).to(dtype)
    off = torch.randn((B, 18, H, W), generator=gen).to(gpu).to(dtype)
    msk = torch.rand((B, 9, H, W), generator=gen).to(gpu).to(dtype)
    with torch.no_grad():
        m(x, off, msk)   # (library and kernels loaded)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = m(x, off, msk)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    print(f"dcn16 {dtype_id(dtype)}: peak rise {rise} bytes, fp32 copies of x and y {4 * (x.numel() + y.numel())} bytes")
    assert rise < 4 * (x.numel() + y.numel())


class _Recorder:
    def __init__(self):
        self.names, self.inner = [], nat.call

    def __call__(self, name, *args):
        self.names.append(name)
        return self.inner(name, *args)


def _problem(cin, cout, dg, dtype, gpu, groups=1, B=2, H=7, W=9, seed=0):
    gen = torch.Generator().manual_seed(seed + cin + cout)
    x = torch.randn((B, cin, H, W), generator=gen).to(gpu).to(dtype)
    w = (torch.randn((cout, cin // groups, 3, 3), generator=gen) * 0.1).to(gpu).to(dtype)
    b = torch.randn((cout,), generator=gen).to(gpu).to(dtype)
    off = (torch.randn((B, dg * 18, H, W), generator=gen) * 1.5).to(gpu).to(dtype)
    msk = torch.rand((B, dg * 9, H, W), generator=gen).to(gpu).to(dtype)
    return x, w, b, off, msk, (3, 3, 1, 1, 1, 1, 1, 1, groups, dg, 64)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_modules_reach_the_16_bit_entry_point_and_two_runs_are_identical(gpu, dtype, monkeypatch):
    g = cases.GEOMETRIES[1]
    case = cases.random_case(g, dtype)
    x, off, msk = (_dev(case[k], dtype, gpu) for k in ("x", "offset", "mask"))
    rec = _Recorder()
    monkeypatch.setattr(nat, "call", rec)
    with torch.no_grad():
        m = _module(case, g, dtype, gpu)
        y1, y2 = m(x, off, msk), m(x, off, msk)
        plain = _module(case, g, None, gpu)          # fp32 parameters under autocast: the weight is rounded once, as .half() rounds it
        with torch.autocast("cuda", dtype=dtype):
            y3 = plain(x, off, msk)
    monkeypatch.setattr(nat, "call", rec.inner)
    assert y1.dtype == dtype and y3.dtype == dtype
    assert torch.equal(y1, y2) and torch.equal(y1, y3)
    assert rec.names.count("fv2p_dcn_forward_h") == 3 and "fv2p_dcn_forward" not in rec.names and "fv2p_dcn_forward_grouped" not in rec.names, rec.names
    assert "fv2p_transpose_batched" not in rec.names, rec.names
    # an empty batch
    with torch.no_grad():
        y0 = m(x[:0], off[:0], msk[:0])
    assert y0.dtype == dtype and tuple(y0.shape) == (0,) + tuple(y1.shape[1:])


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_declined_geometries_fp32_calls_and_the_flag_keep_the_earlier_route(gpu, dtype, monkeypatch):
    rec = _Recorder()
    for cin, cout, dg, groups in [(16, 24, 2, 1), (32, 32, 1, 2)]:   # 8 channels per deformable group; conv groups
        x, w, b, off, msk, conv = _problem(cin, cout, dg, dtype, gpu, groups)
        monkeypatch.setattr(nat, "call", rec)
        del rec.names[:]
        got = DCN.modulated_deform_conv_forward(x, w, b, off, msk, *conv)
        monkeypatch.setattr(nat, "call", rec.inner)
        assert "fv2p_dcn_forward_h" not in rec.names and "fv2p_dcn_forward_grouped" in rec.names, rec.names
        monkeypatch.setattr(DCN, "NATIVE_16BIT", False)
        want = DCN.modulated_deform_conv_forward(x, w, b, off, msk, *conv)
        monkeypatch.setattr(DCN, "NATIVE_16BIT", True)
        assert got.dtype == dtype and torch.equal(got, want)
    # a supported geometry: fp32 tensors and the flag both keep fv2p_dcn_forward
    x, w, b, off, msk, conv = _problem(32, 48, 2, dtype, gpu)
    monkeypatch.setattr(nat, "call", rec)
    del rec.names[:]
    y32 = DCN.modulated_deform_conv_forward(x.float(), w.float(), b.float(), off.float(), msk.float(), *conv)
    assert rec.names == ["fv2p_transpose_batched", "fv2p_dcn_forward", "fv2p_transpose_batched"], rec.names
    del rec.names[:]
    monkeypatch.setattr(DCN, "NATIVE_16BIT", False)
    off_route = DCN.modulated_deform_conv_forward(x, w, b, off, msk, *conv)
    assert "fv2p_dcn_forward" in rec.names and "fv2p_dcn_forward_h" not in rec.names, rec.names
    monkeypatch.setattr(DCN, "NATIVE_16BIT", True)
    del rec.names[:]
    native = DCN.modulated_deform_conv_forward(x, w, b, off, msk, *conv)
    assert "fv2p_dcn_forward_h" in rec.names and "fv2p_dcn_forward" not in rec.names, rec.names
    monkeypatch.setattr(nat, "call", rec.inner)
    assert y32.dtype == torch.float32 and off_route.dtype == dtype and native.dtype == dtype
    assert torch.equal(off_route, y32.to(dtype))   # the earlier route: the fp32 op on the widened tensors, rounded once


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_backward_after_a_native_forward_gives_the_fp32_backwards_gradients(gpu, dtype, monkeypatch):
    g = cases.GEOMETRIES[1]
    case = cases.random_case(g, dtype)
    _, _, dg, _, stride, dil = g
    m = _module(case, g, dtype, gpu)
    x, off, msk = (_dev(case[k], dtype, gpu).requires_grad_(True) for k in ("x", "offset", "mask"))
    rec = _Recorder()
    monkeypatch.setattr(nat, "call", rec)
    y = m(x, off, msk)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).to(gpu).to(dtype)
    y.backward(gy)
    monkeypatch.setattr(nat, "call", rec.inner)
    assert rec.names.count("fv2p_dcn_forward_h") == 1 and rec.names.count("fv2p_dcn_backward") == 1, rec.names
    assert rec.names.count("fv2p_transpose_batched_widen") == 2 and rec.names.count("fv2p_transpose_batched_round") == 1, rec.names
    assert "fv2p_transpose_batched" not in rec.names, rec.names
    conv = (3, 3, stride, stride, dil, dil, dil, dil, 1, dg, 64)
    want = DCN.modulated_deform_conv_backward(x.detach().float(), m.weight.detach().float(), m.bias.detach().float(), off.detach().float(),
                                              msk.detach().float(), gy.float(), *conv)
    assert all(t.dtype == torch.float32 for t in want)
    for name, got, ref in zip(("input", "offset", "mask", "weight", "bias"), (x.grad, off.grad, msk.grad, m.weight.grad, m.bias.grad), want):
        assert got.dtype == dtype and torch.equal(got, ref.to(dtype)), name
    # the raw backward hands grad_input over in the input's dtype and format
    direct = DCN.modulated_deform_conv_backward(x.detach(), m.weight.detach(), m.bias.detach(), off.detach(), msk.detach(), gy, *conv)
    assert direct[0].dtype == dtype and direct[0].is_contiguous() and torch.equal(direct[0], want[0].to(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_conversion_transposes_equal_their_two_step_forms_on_ragged_sizes(gpu, dtype):
    gen = torch.Generator().manual_seed(11)
    for rows in (1, 7, 64, 65):
        for cols in (1, 63, 64, 200):
            src16 = (torch.randn((2, rows, cols), generator=gen) * 3.0).to(gpu).to(dtype)
            src32 = (torch.randn((2, rows, cols), generator=gen) * 3.0).to(gpu)
            two32 = torch.empty((2, cols, rows), dtype=torch.float32, device=gpu)
            nat.call("fv2p_transpose_batched", src16.float(), 2, rows, cols, two32, nat.stream())
            one32 = torch.full((2, cols, rows), float("nan"), dtype=torch.float32, device=gpu)
            nat.call("fv2p_transpose_batched_widen", src16, DT_CODE[dtype], 2, rows, cols, one32, nat.stream())
            assert torch.equal(one32, two32) and torch.equal(one32, src16.float().transpose(1, 2)), (rows, cols)
            nat.call("fv2p_transpose_batched", src32, 2, rows, cols, two32, nat.stream())
            one16 = torch.full((2, cols, rows), float("nan"), dtype=dtype, device=gpu)
            nat.call("fv2p_transpose_batched_round", src32, 2, rows, cols, one16, DT_CODE[dtype], nat.stream())
            assert torch.equal(one16, two32.to(dtype)), (rows, cols)
