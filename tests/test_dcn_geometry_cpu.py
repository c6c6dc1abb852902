"""Deformable convolution geometries without a GPU: which C-ABI entry point every geometry reaches and with which arguments.  Today's
geometries (groups == 1, Cout <= 256, Cin / deformable_group a multiple of 16) reach fv2p_dcn_forward / fv2p_dcn_backward unchanged;
conv groups, channel tails and wide outputs reach fv2p_dcn_*_grouped with the channels padded and the weights in the layouts
include/fv2p_ops.h documents.  The library calls are recorded, not executed (the recorder answers the grouped backward by copying its
inputs into the gradients, so the slicing back to the real channels is checked too)."""
import contextlib
import math

import pytest
import torch

import fv2p_native as _nat
from pcdet.ops.DeformableConvolutionV2PyTorch import DCN
from pcdet.ops.DeformableConvolutionV2PyTorch.modules.modulated_deform_conv import ModulatedDeformConvPack

NEW = ["fv2p_dcn_forward_grouped", "fv2p_dcn_backward_grouped", "fv2p_dcn_backward_grouped_ws_bytes"]


def test_new_entry_points_are_declared_exported_and_sized():
    declared = _nat.declared_symbols()
    lib = _nat.lib()
    for name in NEW:
        assert name in declared, name
        getattr(lib, name)
    # (batch, H, W, Ho, Wo, Cin, Cout, kh, kw, dg, group)
    one = lib.fv2p_dcn_backward_grouped_ws_bytes(1, 20, 24, 20, 24, 96, 64, 3, 3, 2, 3)
    assert one > 0
    assert lib.fv2p_dcn_backward_grouped_ws_bytes(4, 20, 24, 20, 24, 96, 64, 3, 3, 2, 3) > one
    # group 1: the existing query's size
    assert lib.fv2p_dcn_backward_grouped_ws_bytes(2, 20, 24, 20, 24, 64, 64, 3, 3, 4, 1) == lib.fv2p_dcn_backward_ws_bytes(2, 20, 24, 20, 24, 64, 64, 3, 3, 4)


@pytest.fixture
def recorded(monkeypatch):
    """Every library call answered by a recorder: (name, args) in order."""
    calls = []

    def call(name, *args):
        calls.append((name, args))
        if name == "fv2p_dcn_backward_grouped":   # x, wt, offset, mask, dy, 16 geometry ints, group, dx, doffset, dmask, dwt, ...
            args[22].copy_(args[0])
            args[25].copy_(args[1])
        return 0
    monkeypatch.setattr(_nat, "call", call)
    monkeypatch.setattr(_nat, "workspace", lambda nbytes, dev: torch.empty(16, dtype=torch.uint8))
    monkeypatch.setattr(_nat, "stream", lambda: 0)
    monkeypatch.setattr(_nat, "require_cuda", lambda *a: None)
    monkeypatch.setattr(_nat, "device_guard", lambda dev: contextlib.nullcontext())
    return calls


def _problem(cin, cout, group, dg, B=2, H=6, W=7, k=3, stride=1, pad=1, dil=1):
    torch.manual_seed(cin * 7 + cout + group + dg)
    Ho = (H + 2 * pad - (dil * (k - 1) + 1)) // stride + 1
    Wo = (W + 2 * pad - (dil * (k - 1) + 1)) // stride + 1
    x = torch.randn(B, cin, H, W)
    w = torch.randn(cout, cin // group, k, k)
    b = torch.randn(cout)
    off = torch.randn(B, dg * 2 * k * k, Ho, Wo)
    mask = torch.rand(B, dg * k * k, Ho, Wo)
    dy = torch.randn(B, cout, Ho, Wo)
    conv = (k, k, stride, stride, pad, pad, dil, dil, group, dg, 64)
    return x, w, b, off, mask, dy, conv, (B, H, W, Ho, Wo)


def _padded(cin, group, dg):
    s = math.gcd(cin // group, cin // dg)
    sp = -(-s // 16) * 16
    return s, sp, cin // s * sp


def _pad_ref(t, s, sp):
    """Last axis in pieces of s, each followed by sp - s zeros (written out with a loop, independently of DCN._tail_pad)."""
    out = torch.zeros(*t.shape[:-1], t.shape[-1] // s * sp, dtype=t.dtype)
    for j in range(t.shape[-1] // s):
        out[..., j * sp:j * sp + s] = t[..., j * s:(j + 1) * s]
    return out


@pytest.mark.parametrize("cin,cout,dg", [(32, 48, 2), (16, 16, 1), (64, 256, 4), (32, 50, 1)])
def test_todays_geometries_reach_the_existing_entry_points_unchanged(recorded, cin, cout, dg):
    x, w, b, off, mask, dy, conv, (B, H, W, Ho, Wo) = _problem(cin, cout, 1, dg)
    DCN.modulated_deform_conv_forward(x, w, b, off, mask, *conv)
    DCN.modulated_deform_conv_backward(x, w, b, off, mask, dy, *conv)
    DCN.deform_conv_forward(x, w, b, off, *conv)
    assert [n for n, _ in recorded] == ["fv2p_dcn_forward", "fv2p_dcn_backward", "fv2p_dcn_forward"]
    geom = (B, H, W, cin, cout, Ho, Wo, 3, 3, 1, 1, 1, 1, 1, 1, dg)
    _, a = recorded[0]
    assert a[5:21] == geom and len(a) == 23
    assert torch.equal(a[0], x.permute(0, 2, 3, 1)) and torch.equal(a[1], DCN._wt_oc(w)) and torch.equal(a[2], b)
    _, a = recorded[1]
    cp = cout + (-cout) % 4
    assert a[5:21] == geom[:4] + (cp,) + geom[5:] and len(a) == 28
    assert torch.equal(a[1], torch.nn.functional.pad(DCN._wt(w), (0, cp - cout)))
    assert a[4].shape == (B * Ho * Wo, cp)


@pytest.mark.parametrize("cin,cout,group,dg", [
    (32, 32, 2, 2), (64, 32, 2, 4), (64, 64, 4, 2), (48, 48, 3, 2), (16, 16, 16, 1), (32, 24, 2, 1), (32, 18, 2, 2),
    (3, 8, 1, 1), (4, 6, 1, 2), (24, 16, 1, 3), (40, 16, 1, 1), (8, 16, 1, 8),
    (16, 300, 1, 1), (32, 512, 2, 1)])
def test_new_geometries_reach_the_grouped_entry_points(recorded, cin, cout, group, dg):
    x, w, b, off, mask, dy, conv, (B, H, W, Ho, Wo) = _problem(cin, cout, group, dg)
    s, sp, cpad = _padded(cin, group, dg)
    cing = cpad // group
    DCN.modulated_deform_conv_forward(x, w, b, off, mask, *conv)
    gi, go, gm, gw, gb = DCN.modulated_deform_conv_backward(x, w, b, off, mask, dy, *conv)
    assert [n for n, _ in recorded] == ["fv2p_dcn_forward_grouped", "fv2p_dcn_backward_grouped"]
    # forward: x NHWC padded, wt_oc [K][Cout][Cin'/G], geometry with the padded channels, then the group count
    _, a = recorded[0]
    assert a[5:22] == (B, H, W, cpad, cout, Ho, Wo, 3, 3, 1, 1, 1, 1, 1, 1, dg, group) and len(a) == 24
    assert torch.equal(a[0], _pad_ref(x.permute(0, 2, 3, 1), s, sp))
    assert torch.equal(a[1], _pad_ref(w.permute(2, 3, 0, 1), s, sp).reshape(9, cout, cing))
    assert torch.equal(a[2], b) and a[3] is not None and a[22].shape == (B * Ho * Wo, cout)
    # backward: wt [K][Cin'][Cout'/G] with wt[k][g*cing + c][o] = W[g*coutg + o, c, k], each group's columns padded to 4
    _, a = recorded[1]
    coutg = cout // group
    cop = coutg + (-coutg) % 4
    assert a[5:22] == (B, H, W, cpad, group * cop, Ho, Wo, 3, 3, 1, 1, 1, 1, 1, 1, dg, group) and len(a) == 29
    wp = _pad_ref(w.permute(0, 2, 3, 1), s, sp).reshape(cout, 9, cing)
    want = torch.zeros(9, cpad, cop)
    for o in range(cout):
        gg, ol = divmod(o, coutg)
        want[:, gg * cing:(gg + 1) * cing, ol] = wp[o]
    assert torch.equal(a[1], want)
    assert a[4].shape == (B * Ho * Wo, group * cop)
    assert torch.equal(a[4].view(-1, group, cop)[..., :coutg].reshape(-1, cout), dy.permute(0, 2, 3, 1).reshape(-1, cout))
    assert a[25].shape == (9, cpad, cop) and a[22].shape == (B, H, W, cpad)
    # the recorder handed x and wt back as dx and dwt: sliced back to the real channels they are the input and the weight again
    assert torch.equal(gi, x) and torch.equal(gw, w)
    assert torch.allclose(gb, dy.sum(dim=(0, 2, 3)), rtol=1e-5, atol=1e-5)
    assert go.shape == off.shape and gm.shape == mask.shape


def test_module_with_a_channel_tail_reaches_the_grouped_entry_points(recorded):
    """ModulatedDeformConvPack(4, 6, 3, deformable_groups=2): 2 channels per deformable group, each padded to 16."""
    m = ModulatedDeformConvPack(4, 6, 3, stride=1, padding=1, deformable_groups=2)
    x = torch.randn(2, 4, 5, 6, requires_grad=True)
    recorded.clear()
    y = m(x)
    assert y.shape == (2, 6, 5, 6)
    names = [n for n, _ in recorded]
    assert names == ["fv2p_dcn_forward_grouped"]
    assert recorded[0][1][5:22] == (2, 5, 6, 32, 6, 5, 6, 3, 3, 1, 1, 1, 1, 1, 1, 2, 1)


def test_channels_last_input_keeps_its_format_on_the_grouped_route(recorded):
    x, w, b, off, mask, dy, conv, _ = _problem(32, 32, 2, 2)
    xc = x.contiguous(memory_format=torch.channels_last)
    y = DCN.modulated_deform_conv_forward(xc, w, b, off, mask, *conv)
    assert y.is_contiguous(memory_format=torch.channels_last)
    gi = DCN.modulated_deform_conv_backward(xc, w, b, off, mask, dy, *conv)[0]
    assert gi.is_contiguous(memory_format=torch.channels_last) and torch.equal(gi, x)


@pytest.mark.parametrize("cin,cout,group,dg,wshape", [
    (30, 32, 4, 1, None),          # Cin % G
    (32, 30, 4, 1, None),          # Cout % G
    (32, 32, 1, 3, None),          # Cin % dg
    (32, 32, 2, 1, (32, 32, 3, 3)),  # a group-1 weight for a grouped call
    (32, 32, 2, 1, (32, 16, 3, 1)),  # kernel size
])
def test_invalid_geometries_raise(recorded, cin, cout, group, dg, wshape):
    x = torch.randn(1, cin, 5, 5)
    w = torch.randn(*(wshape or (cout, cin // group if cin % group == 0 else 1, 3, 3)))
    off, mask = torch.randn(1, dg * 18, 5, 5), torch.rand(1, dg * 9, 5, 5)
    conv = (3, 3, 1, 1, 1, 1, 1, 1, group, dg, 64)
    with pytest.raises(ValueError):
        DCN.modulated_deform_conv_forward(x, w, None, off, mask, *conv)
    with pytest.raises(ValueError):
        DCN.modulated_deform_conv_backward(x, w, None, off, mask, torch.randn(1, cout, 5, 5), *conv)
    assert recorded == []


def test_cpu_tensor_still_raises_on_the_grouped_route():
    x, w, b, off, mask, dy, conv, _ = _problem(32, 32, 2, 2)
    with pytest.raises(Exception):
        DCN.modulated_deform_conv_forward(x, w, b, off, mask, *conv)


@pytest.mark.parametrize("s,sp", [(1, 16), (3, 16), (8, 16), (24, 32)])
def test_tail_unpad_is_a_contiguous_inverse(s, sp):
    """The unpadded gradient goes to the library's NHWC -> NCHW transpose, which reads it as contiguous: with 1-channel pieces the
    reshape alone would be a strided view."""
    t = torch.randn(2, 3, 4, 5 * s)
    p = DCN._tail_pad(t, (s, sp))
    assert p.shape == (2, 3, 4, 5 * sp) and torch.equal(p, _pad_ref(t, s, sp))
    u = DCN._tail_unpad(p, (s, sp))
    assert u.is_contiguous() and torch.equal(u, t)
