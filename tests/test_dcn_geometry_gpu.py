"""GPU parity of the deformable convolution over the geometries of the reference beyond fv2p_dcn_forward / _backward: conv groups
(modulated_deform_conv_cuda.cu:62-113, 171-280: one GEMM per group), channels per deformable group that are not a multiple of 16
(zero-padded on the host), and more than 256 output channels.

The float64 reference is the oracle, unchanged, called with the block-diagonal dense weight Wd[o, c] = W[o, c - g*Cin/G] for c in o's
group g and 0 elsewhere: that is the grouped operator exactly, and autograd gives the weight gradient as Wd's diagonal blocks.
Tolerances as test_dcn_gpu.py: forward and all five gradients 1e-4 relative to the largest entry.  Every backward runs twice and gives
the same bits (no float atomics on any path)."""
import pytest
import torch

import fv2p_native
from oracle import dcn_oracle
from pcdet.ops.DeformableConvolutionV2PyTorch import DCN
from pcdet.ops.DeformableConvolutionV2PyTorch.functions import DeformConvFunction, ModulatedDeformConvFunction
from pcdet.ops.DeformableConvolutionV2PyTorch.modules.deform_conv import DeformConv
from pcdet.ops.DeformableConvolutionV2PyTorch.modules.modulated_deform_conv import ModulatedDeformConv, ModulatedDeformConvPack

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def dense(w, group, cin):
    """[Cout, Cin/G, kh, kw] -> block-diagonal [Cout, Cin, kh, kw] (differentiable: w.grad = the diagonal blocks of the dense gradient)."""
    cout = w.shape[0]
    coutg, cing = cout // group, cin // group
    wd = w.new_zeros((cout, cin) + tuple(w.shape[2:]))
    for g in range(group):
        wd[g * coutg:(g + 1) * coutg, g * cing:(g + 1) * cing] = w[g * coutg:(g + 1) * coutg]
    return wd


def check(gpu, cin, cout, group, dg, B=2, H=9, W=10, stride=1, dil=1, v1=False, scale=1.5, seed=0):
    """Forward and every gradient against the float64 oracle; the backward twice, bit for bit."""
    torch.manual_seed(seed)
    pad = dil
    Ho, Wo = (H + 2 * pad - (dil * 2 + 1)) // stride + 1, (W + 2 * pad - (dil * 2 + 1)) // stride + 1
    x = torch.randn(B, cin, H, W)
    offset = torch.randn(B, dg * 18, Ho, Wo) * scale     # leaves the map often: the border rule
    mask = torch.ones(B, dg * 9, Ho, Wo) if v1 else torch.sigmoid(torch.randn(B, dg * 9, Ho, Wo))
    w = torch.randn(cout, cin // group, 3, 3) * 0.2
    b = torch.zeros(cout) if v1 else torch.randn(cout)
    g = torch.randn(B, cout, Ho, Wo)

    def run():
        leaves = [t.clone().to(gpu).requires_grad_(True) for t in ((x, offset) if v1 else (x, offset, mask))] + \
                 [t.clone().to(gpu).requires_grad_(True) for t in (w, b)]
        if v1:
            gx, go, gw, gb = leaves
            y = DeformConvFunction.apply(gx, go, gw, gb, stride, pad, dil, group, dg, 64)
        else:
            gx, go, gm, gw, gb = leaves
            y = ModulatedDeformConvFunction.apply(gx, go, gm, gw, gb, stride, pad, dil, group, dg, 64)
        y.backward(g.to(gpu))
        return [y.detach()] + [t.grad.detach().clone() for t in leaves]

    got = run()
    again = run()
    for a, b_ in zip(got[1:], again[1:]):
        assert torch.equal(a, b_), "backward differs between two runs"
    cx, co, cm = (t.clone().double().requires_grad_(True) for t in (x, offset, mask))
    cw, cb = w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = dcn_oracle.modulated_deform_conv(cx, co, cm, dense(cw, group, cin), cb, (stride, stride), (pad, pad), (dil, dil), dg)
    ref.backward(g.double())
    want = [ref, cx.grad, co.grad] + ([] if v1 else [cm.grad]) + [cw.grad, cb.grad]
    names = ["y", "dx", "doffset"] + ([] if v1 else ["dmask"]) + ["dweight", "dbias"]
    for name, a, r in zip(names, got, want):
        assert a.shape == r.shape, name
        assert rel(a, r) < 1e-4, (name, rel(a, r))
    return got


@pytest.mark.parametrize("cin,cout,group,dg,stride,dil", [
    (32, 32, 2, 2, 1, 1),     # G = dg
    (64, 32, 2, 4, 1, 1),     # dg a multiple of G
    (64, 64, 4, 2, 1, 1),     # G a multiple of dg: a deformable group spans two conv groups
    (48, 48, 3, 2, 1, 1),     # neither; 8-channel pieces padded to 16
    (16, 16, 16, 1, 1, 1),    # depthwise
    (32, 24, 2, 1, 1, 1),     # Cout/G = 12: not a multiple of 16
    (32, 18, 2, 2, 1, 1),     # Cout/G = 9: not a multiple of 4
    (64, 64, 2, 4, 2, 1),     # stride 2
    (48, 48, 3, 2, 1, 2),     # dilation 2
])
@pytest.mark.parametrize("v1", [False, True], ids=["dcnv2", "dcnv1"])
def test_groups_vs_oracle(gpu, cin, cout, group, dg, stride, dil, v1):
    check(gpu, cin, cout, group, dg, stride=stride, dil=dil, v1=v1)


@pytest.mark.parametrize("cin,cout,group,dg", [(48, 48, 3, 2), (64, 64, 4, 2), (64, 32, 2, 4), (32, 300, 1, 2)])
@pytest.mark.parametrize("order", [0, 1], ids=["tap-outer", "tap-inner"])
def test_grouped_forward_step_orders_vs_oracle(gpu, cin, cout, group, dg, order):
    try:
        fv2p_native.call("fv2p_dcn_set_forward_order", order)
        check(gpu, cin, cout, group, dg, seed=order + 1)
    finally:
        fv2p_native.call("fv2p_dcn_set_forward_order", -1)


@pytest.mark.parametrize("cin,cout,dg", [(3, 8, 3), (3, 16, 1), (16, 16, 2), (24, 32, 1), (40, 16, 1), (48, 32, 2)],
                         ids=["cpg1", "rgb", "cpg8", "cpg24", "cpg40", "cpg24x2"])
@pytest.mark.parametrize("v1", [False, True], ids=["dcnv2", "dcnv1"])
def test_channel_tails_vs_oracle(gpu, cin, cout, dg, v1):
    check(gpu, cin, cout, 1, dg, v1=v1)


@pytest.mark.parametrize("cin,cout,group,dg", [(16, 257, 1, 1), (16, 300, 1, 1), (32, 512, 1, 2), (32, 1024, 2, 1)])
def test_wide_output_vs_oracle(gpu, cin, cout, group, dg):
    check(gpu, cin, cout, group, dg, B=2, H=6, W=7)


@pytest.mark.parametrize("cin,cout,group,dg,per_chunk", [(48, 48, 3, 2, 2), (64, 64, 4, 2, 1), (16, 300, 1, 1, 3)])
def test_grouped_backward_in_batch_chunks(gpu, cin, cout, group, dg, per_chunk):
    """fv2p_dcn_set_colg_cap lowered: the grouped backward of a batch of 5 runs in chunks.  Input, offset and mask gradients are the
    same bits as the whole call (per-sample work), the weight gradient within 1e-6 (chunks added in ascending order)."""
    torch.manual_seed(per_chunk)
    B, H, W = 5, 11, 13
    x = torch.randn(B, cin, H, W, device=gpu)
    offset = torch.randn(B, dg * 18, H, W, device=gpu) * 1.5
    mask = torch.sigmoid(torch.randn(B, dg * 9, H, W, device=gpu))
    w = torch.randn(cout, cin // group, 3, 3, device=gpu) * 0.2
    b = torch.randn(cout, device=gpu)
    dy = torch.randn(B, cout, H, W, device=gpu)
    args = (3, 3, 1, 1, 1, 1, 1, 1, group, dg, 64)
    whole = DCN.modulated_deform_conv_backward(x, w, b, offset, mask, dy, *args)
    cpad = DCN._geom_grouped(x, w, *args[:10])[0][3]
    try:
        fv2p_native.call("fv2p_dcn_set_colg_cap", per_chunk * H * W * 9 * cpad * 4)
        parts = DCN.modulated_deform_conv_backward(x, w, b, offset, mask, dy, *args)
        again = DCN.modulated_deform_conv_backward(x, w, b, offset, mask, dy, *args)
    finally:
        fv2p_native.call("fv2p_dcn_set_colg_cap", 0)
    for i in range(3):
        assert torch.equal(parts[i], whole[i]), i
    assert rel(parts[3], whole[3]) < 1e-6
    for a, b_ in zip(parts, again):
        assert torch.equal(a, b_)


@pytest.mark.parametrize("cin,cout,dg", [(16, 16, 1), (64, 32, 4), (128, 128, 1), (32, 200, 2), (32, 48, 2), (32, 50, 1)])
def test_group_one_grouped_entry_points_match_the_existing_ones(gpu, cin, cout, dg):
    """On the shapes of test_dcn_gpu.py: fv2p_dcn_*_grouped with group = 1 run today's kernels and give today's bits."""
    torch.manual_seed(cin + cout)
    B, H, W = 2, 11, 13
    x = torch.randn(B, H, W, cin, device=gpu)
    offset = torch.randn(B, dg * 18, H, W, device=gpu) * 1.5
    mask = torch.sigmoid(torch.randn(B, dg * 9, H, W, device=gpu))
    w = torch.randn(cout, cin, 3, 3, device=gpu) * 0.2
    bias = torch.randn(cout, device=gpu)
    geom = (B, H, W, cin, cout, H, W, 3, 3, 1, 1, 1, 1, 1, 1, dg)
    stream = fv2p_native.stream()
    for order in (0, 1):
        try:
            fv2p_native.call("fv2p_dcn_set_forward_order", order)
            y0 = torch.empty(B * H * W, cout, device=gpu)
            y1 = torch.empty_like(y0)
            fv2p_native.call("fv2p_dcn_forward", x, DCN._wt_oc(w), bias, offset, mask, *geom, y0, stream)
            fv2p_native.call("fv2p_dcn_forward_grouped", x, DCN._wt_oc(w), bias, offset, mask, *geom, 1, y1, stream)
        finally:
            fv2p_native.call("fv2p_dcn_set_forward_order", -1)
        assert torch.equal(y0, y1), order
    cp = cout + (-cout) % 4
    wt = torch.nn.functional.pad(DCN._wt(w), (0, cp - cout))
    dy = torch.nn.functional.pad(torch.randn(B * H * W, cout, device=gpu), (0, cp - cout))
    g = geom[:4] + (cp,) + geom[5:]
    lib = fv2p_native.lib()
    nb = lib.fv2p_dcn_backward_ws_bytes(B, H, W, H, W, cin, cp, 3, 3, dg)
    assert lib.fv2p_dcn_backward_grouped_ws_bytes(B, H, W, H, W, cin, cp, 3, 3, dg, 1) == nb
    outs = []
    for name, extra in (("fv2p_dcn_backward", ()), ("fv2p_dcn_backward_grouped", (1,))):
        dx = torch.empty_like(x)
        doff, dmask = torch.empty_like(offset), torch.empty_like(mask)
        dwt = torch.empty(9, cin, cp, device=gpu)
        ws = torch.empty(nb, dtype=torch.uint8, device=gpu)
        fv2p_native.call(name, x, wt, offset, mask, dy, *g, *extra, dx, doff, dmask, dwt, ws, ws.numel(), stream)
        outs.append((dx, doff, dmask, dwt))
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_)


def test_grouped_entry_points_refuse_what_the_kernels_cannot_take(gpu):
    """Cin/G or Cin/dg not a multiple of 16 (the caller pads), G not dividing the channels, Cout/G not a multiple of 4 (backward)."""
    x = torch.zeros(1, 5, 5, 48, device=gpu)
    off, mask = torch.zeros(1, 36, 5, 5, device=gpu), torch.zeros(1, 18, 5, 5, device=gpu)
    y = torch.empty(25, 48, device=gpu)
    s = fv2p_native.stream()
    for dg, group in ((2, 3), (1, 5)):
        geom = (1, 5, 5, 48, 48, 5, 5, 3, 3, 1, 1, 1, 1, 1, 1, dg)
        with pytest.raises(Exception):
            fv2p_native.call("fv2p_dcn_forward_grouped", x, torch.zeros(9, 48, 48 // group, device=gpu), None, off[:, :dg * 18],
                             mask[:, :dg * 9], *geom, group, y, s)


def test_modules_with_groups(gpu):
    """ModulatedDeformConv / DeformConv / ModulatedDeformConvPack with groups = 2: forward and backward against the oracle, and a
    channels-last input keeps its format on the grouped route."""
    torch.manual_seed(5)
    B, C, H, W = 2, 32, 8, 9
    x = torch.randn(B, C, H, W)
    offset = torch.randn(B, 18, H, W)
    mask = torch.sigmoid(torch.randn(B, 9, H, W))
    m = ModulatedDeformConv(C, 48, 3, 1, 1, groups=2).to(gpu)
    d = DeformConv(C, 48, 3, 1, 1, groups=2, bias=False).to(gpu)
    gx = x.clone().to(gpu).requires_grad_(True)
    y = m(gx, offset.to(gpu), mask.to(gpu))
    cx = x.clone().double().requires_grad_(True)
    cw = m.weight.detach().cpu().double().requires_grad_(True)
    ref = dcn_oracle.modulated_deform_conv(cx, offset.double(), mask.double(), dense(cw, 2, C), m.bias.detach().cpu().double(),
                                           (1, 1), (1, 1), (1, 1), 1)
    assert rel(y, ref) < 1e-4
    y.square().sum().backward()
    ref.square().sum().backward()
    assert rel(gx.grad, cx.grad) < 1e-4 and rel(m.weight.grad, cw.grad) < 1e-4
    yd = d(x.to(gpu), offset.to(gpu))
    refd = dcn_oracle.modulated_deform_conv(x.double(), offset.double(), torch.ones(B, 9, H, W, dtype=torch.float64),
                                            dense(d.weight.detach().cpu().double(), 2, C), d.bias.detach().cpu().double(),
                                            (1, 1), (1, 1), (1, 1), 1)
    assert rel(yd, refd) < 1e-4
    p = ModulatedDeformConvPack(C, 48, 3, 1, 1, groups=2, deformable_groups=2).to(gpu)
    xp = x.to(gpu).requires_grad_(True)
    p(xp).sum().backward()
    assert torch.isfinite(xp.grad).all() and torch.isfinite(p.weight.grad).all() and p.weight.grad.shape == (48, 16, 3, 3)
    # channels-last in, channels-last out, and its grad_input too
    xc = x.to(gpu).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    yc = m(xc, offset.to(gpu), mask.to(gpu))
    assert yc.is_contiguous(memory_format=torch.channels_last)
    assert rel(yc, ref) < 1e-4
    yc.square().sum().backward()
    assert xc.grad.is_contiguous(memory_format=torch.channels_last) and rel(xc.grad, cx.grad) < 1e-4


def test_pack_with_a_channel_tail(gpu):
    """ModulatedDeformConvPack(4, 6, 3, deformable_groups=2): two channels per deformable group (each padded to 16 on the way in)."""
    torch.manual_seed(7)
    p = ModulatedDeformConvPack(4, 6, 3, 1, 1, deformable_groups=2).to(gpu)
    with torch.no_grad():
        p.conv_offset_mask.weight.normal_(0, 0.3)     # (zero-initialised: make the offsets and the mask non-trivial)
    x = torch.randn(2, 4, 10, 11, device=gpu, requires_grad=True)
    y = p(x)
    om = p.conv_offset_mask(x).detach().cpu().double()
    o1, o2, mk = torch.chunk(om, 3, dim=1)
    cx = x.detach().cpu().double().requires_grad_(True)
    cw = p.weight.detach().cpu().double().requires_grad_(True)
    ref = dcn_oracle.modulated_deform_conv(cx, torch.cat((o1, o2), 1), torch.sigmoid(mk), cw, p.bias.detach().cpu().double(),
                                           (1, 1), (1, 1), (1, 1), 2)
    assert y.shape == ref.shape and rel(y, ref) < 1e-4
