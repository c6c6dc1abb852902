"""`DCN` — the extension module of the reference's DeformableConvolutionV2PyTorch (src/vision.cpp:6-12) as a Python
shim over libfv2p_ops: same six function names and positional arguments.

Two routes.  groups == 1, Cout <= 256 and Cin / deformable_group a multiple of 16 (every reference config, the MGAF head) reach
fv2p_dcn_forward / fv2p_dcn_backward as they always did.  Every other geometry the reference accepts (groups > 1, channel tails,
Cout > 256) reaches fv2p_dcn_*_grouped, with the input channels zero-padded on the host (_tail_pad).

float16 / bfloat16 maps: the forward of groups == 1 with Cin / deformable_group a multiple of 16 reaches fv2p_dcn_forward_h, the same
implicit GEMM on the 16-bit MFMA with no fp32 copy of any map (NATIVE_16BIT, on by default; off = the fp32 route on widened copies, as
before).  The backward keeps the fp32 kernels by default and reaches them through fv2p_transpose_batched_widen / _round: the layout copy
and the dtype copy of x, grad_output and grad_input are one pass each.  NATIVE_16BIT_BACKWARD (off by default) sends the backward of the
same calls with Cout <= 256 to fv2p_dcn_backward_h instead: x, grad_output, the weight, the column gradients and grad_input stay in 16
bits, grad_offset / grad_mask come in the offsets' dtype and grad_weight from an fp32 buffer (csrc/dcn_bwd_h.hip)."""
import math

import torch

import fv2p_native as _nat

NATIVE_16BIT = True    # float16 / bfloat16 forward on fv2p_dcn_forward_h where it serves the geometry; False: the fp32 kernels on widened copies
NATIVE_16BIT_BACKWARD = False   # float16 / bfloat16 backward on fv2p_dcn_backward_h where it serves the geometry; False: the fp32 kernels on widened copies
_DT16 = {torch.float16: 1, torch.bfloat16: 2}   # FV2P_DT_F16 / FV2P_DT_BF16


def _geom(input, weight, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, deformable_group):
    _nat.require_cuda(input)  # raises on a CPU tensor, as the reference dispatcher does ("Not implemented on the CPU", modulated_deform_conv.h:43)
    if group != 1:
        raise NotImplementedError("fv2p DCN: groups > 1 is not supported (no reference config uses it)")
    B, C, H, W = input.shape
    Cout = weight.shape[0]
    assert weight.shape[1] == C and weight.shape[2] == kernel_h and weight.shape[3] == kernel_w, "input / kernel shape mismatch"
    Ho = (H + 2 * pad_h - (dilation_h * (kernel_h - 1) + 1)) // stride_h + 1
    Wo = (W + 2 * pad_w - (dilation_w * (kernel_w - 1) + 1)) // stride_w + 1
    return (B, H, W, C, Cout, Ho, Wo, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group)


def _plain(input, weight, group, deformable_group):
    """The geometries fv2p_dcn_forward / fv2p_dcn_backward take: today's route, unchanged."""
    C, Cout = input.shape[1], weight.shape[0]
    return group == 1 and Cout <= 256 and deformable_group >= 1 and C % deformable_group == 0 and (C // deformable_group) % 16 == 0


def _geom_grouped(input, weight, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, deformable_group):
    """-> (geometry of the padded problem, (s, sp)): the reference's checks (modulated_deform_conv_cuda.cu:40-58), then the channel
    padding.  The input channels split at every conv-group and every deformable-group boundary into pieces s = gcd(Cin/G, Cin/dg)
    wide; each piece is zero-padded to sp = s rounded up to 16, so that both kinds of group hold a multiple of 16 channels."""
    _nat.require_cuda(input)
    B, C, H, W = input.shape
    Cout = weight.shape[0]
    if group < 1 or C % group or Cout % group:
        raise ValueError(f"DCN: groups {group} must divide input channels {C} and output channels {Cout}")
    if deformable_group < 1 or C % deformable_group:
        raise ValueError(f"DCN: deformable groups {deformable_group} must divide input channels {C}")
    if tuple(weight.shape[1:]) != (C // group, kernel_h, kernel_w):
        raise ValueError(f"DCN: input / kernel shape mismatch: weight {tuple(weight.shape)} for {C} input channels in {group} groups")
    Ho = (H + 2 * pad_h - (dilation_h * (kernel_h - 1) + 1)) // stride_h + 1
    Wo = (W + 2 * pad_w - (dilation_w * (kernel_w - 1) + 1)) // stride_w + 1
    s = math.gcd(C // group, C // deformable_group)
    sp = -(-s // 16) * 16
    g = (B, H, W, C // s * sp, Cout, Ho, Wo, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group)
    return g, (s, sp)


def _tail_pad(t, tail):
    """Last axis in pieces of s channels, each zero-padded to sp.  The cost is the padding: a piece of 1 channel is moved and
    multiplied 16 times over (sp / s), in x, the weight and the column gradients alike."""
    s, sp = tail
    if s == sp:
        return t
    lead = t.shape[:-1]
    return torch.nn.functional.pad(t.reshape(*lead, t.shape[-1] // s, s), (0, sp - s)).reshape(*lead, t.shape[-1] // s * sp)


def _tail_unpad(t, tail):
    """Inverse of _tail_pad: the real channels of every piece, as a contiguous copy (with s = 1 the reshape alone would be a view with
    a channel stride of sp, which the library's transposes must not see)."""
    s, sp = tail
    if s == sp:
        return t
    lead = t.shape[:-1]
    return t.reshape(*lead, t.shape[-1] // sp, sp)[..., :s].reshape(*lead, t.shape[-1] // sp * s).contiguous()


def _channels_last(t):
    return t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()


def _to_nhwc(t):
    """[B, C, H, W] (any strides) -> contiguous fp32 [B, H, W, C]: a view for a channels-last tensor, the library's tiled transpose for a
    contiguous one (torch's generic strided copy moves these 70 - 150 MB per DCN layer at a fraction of the bandwidth)."""
    t = t.float()
    v = t.permute(0, 2, 3, 1)
    if v.is_contiguous():
        return v
    if t.is_contiguous() and t.is_cuda and t.numel() > 0:
        B, C, H, W = t.shape
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=t.device)
        with _nat.device_guard(t.device):
            _nat.call("fv2p_transpose_batched", t, B, C, H * W, out, _nat.stream())
        return out
    return v.contiguous()


def _to_nchw(t_nhwc):
    """contiguous fp32 [B, H, W, C] -> contiguous [B, C, H, W] (what the reference returns, modulated_deform_conv_cuda.cu:118)."""
    B, H, W, C = t_nhwc.shape
    if not t_nhwc.is_cuda or t_nhwc.numel() == 0:
        return t_nhwc.permute(0, 3, 1, 2).contiguous()
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=t_nhwc.device)
    with _nat.device_guard(t_nhwc.device):
        _nat.call("fv2p_transpose_batched", t_nhwc, B, H * W, C, out, _nat.stream())
    return out


def _to_nhwc_f32(t):
    """_to_nhwc with the widening inside the copy: a contiguous 16-bit [B, C, H, W] -> contiguous fp32 [B, H, W, C] in one pass,
    the bits of t.float() followed by the transpose."""
    if t.dtype in _DT16 and t.is_cuda and t.is_contiguous() and t.numel() > 0 and not t.permute(0, 2, 3, 1).is_contiguous():
        B, C, H, W = t.shape
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=t.device)
        with _nat.device_guard(t.device):
            _nat.call("fv2p_transpose_batched_widen", t, _DT16[t.dtype], B, C, H * W, out, _nat.stream())
        return out
    return _to_nhwc(t)


def _to_nchw_as(t_nhwc, dtype):
    """_to_nchw(t).to(dtype) with the rounding inside the copy for a 16-bit dtype: fp32 [B, H, W, C] -> [B, C, H, W] in one pass."""
    if dtype in _DT16 and t_nhwc.is_cuda and t_nhwc.numel() > 0:
        B, H, W, C = t_nhwc.shape
        out = torch.empty((B, C, H, W), dtype=dtype, device=t_nhwc.device)
        with _nat.device_guard(t_nhwc.device):
            _nat.call("fv2p_transpose_batched_round", t_nhwc, B, H * W, C, out, _DT16[dtype], _nat.stream())
        return out
    return _to_nchw(t_nhwc).to(dtype)


def _native_16bit(input, weight, group, deformable_group):
    """The calls fv2p_dcn_forward_h takes: a float16 / bfloat16 map on the GPU, no conv groups, a geometry the kernel serves."""
    if not (NATIVE_16BIT and input.dtype in _DT16 and input.is_cuda and group == 1 and deformable_group >= 1):
        return False
    return bool(_nat.lib().fv2p_dcn_forward_h_supported(input.shape[1], weight.shape[0], deformable_group))


def _forward_16bit(input, weight, bias, offset, mask, g):
    """fv2p_dcn_forward_h: x, the weight and y in input.dtype, no .float() of any map.  The weight (fp32 master weights under
    autocast) is rounded once while it is permuted; offset and mask go as they are in input.dtype or float32."""
    B, H, W, C, Cout, Ho, Wo = g[:7]
    dt, dev = input.dtype, input.device
    x = input.permute(0, 2, 3, 1)
    if B * H * W > 0 and not x.is_contiguous():
        if input.is_contiguous():
            x = torch.empty((B, H, W, C), dtype=dt, device=dev)
            with _nat.device_guard(dev):
                _nat.call("fv2p_transpose_batched_h", input, B, C, H * W, x, _nat.stream())
        else:
            x = x.contiguous()
    wt_oc = _wt_oc(weight if weight.dtype == dt else weight.to(dt))
    om = offset.dtype if offset.dtype == mask.dtype and offset.dtype in (dt, torch.float32) else torch.float32
    off = (offset if offset.dtype == om else offset.to(om)).contiguous()
    msk = (mask if mask.dtype == om else mask.to(om)).contiguous()
    y = torch.empty((B, Ho, Wo, Cout), dtype=dt, device=dev)
    with _nat.device_guard(dev):
        _nat.call("fv2p_dcn_forward_h", x, wt_oc, bias.float().contiguous() if bias is not None else None, off, msk, *g, y,
                  _DT16[dt], 0 if om == torch.float32 else _DT16[dt], _nat.stream())
        if _channels_last(input) or y.numel() == 0:
            return y.permute(0, 3, 1, 2) if _channels_last(input) else y.permute(0, 3, 1, 2).contiguous()
        out = torch.empty((B, Cout, Ho, Wo), dtype=dt, device=dev)
        _nat.call("fv2p_transpose_batched_h", y, B, Ho * Wo, Cout, out, _nat.stream())
    return out


def _wt(weight):
    """[Cout, Cin, kh, kw] -> [kh*kw][Cin][Cout]: the backward kernels' layout (output channels contiguous)."""
    cout, cin, kh, kw = weight.shape
    return weight.permute(2, 3, 1, 0).reshape(kh * kw, cin, cout).contiguous()


def _wt_oc(weight):
    """[Cout, Cin, kh, kw] -> [kh*kw][Cout][Cin]: the forward kernel's layout (input channels contiguous)."""
    cout, cin, kh, kw = weight.shape
    return weight.permute(2, 3, 0, 1).reshape(kh * kw, cout, cin).contiguous()


def _nhwc_16bit(t):
    """[B, C, H, W] 16-bit (any strides) -> contiguous [B, H, W, C] in the same dtype: a view for a channels-last tensor, else
    fv2p_transpose_batched_h."""
    B, C, H, W = t.shape
    v = t.permute(0, 2, 3, 1)
    if t.numel() == 0 or v.is_contiguous() or not t.is_contiguous():
        return v.contiguous()
    out = torch.empty((B, H, W, C), dtype=t.dtype, device=t.device)
    with _nat.device_guard(t.device):
        _nat.call("fv2p_transpose_batched_h", t, B, C, H * W, out, _nat.stream())
    return out


def _native_16bit_backward(input, weight, group, deformable_group):
    """The calls fv2p_dcn_backward_h takes: a float16 / bfloat16 map on the GPU, no conv groups, the forward's geometry with
    Cout <= 256 (a Cout that is no multiple of 8 is zero-padded on the way in)."""
    if not (NATIVE_16BIT_BACKWARD and input.dtype in _DT16 and input.is_cuda and group == 1 and deformable_group >= 1):
        return False
    cout = weight.shape[0]
    return bool(_nat.lib().fv2p_dcn_backward_h_supported(input.shape[1], cout + (-cout) % 8, deformable_group))


def _backward_16bit(input, weight, offset, mask, grad_output, g):
    """fv2p_dcn_backward_h: x, grad_output, the weight and grad_input in input.dtype, no .float() of any map.  The weight (fp32 master
    weights under autocast) is rounded once while it is permuted; offset and mask go as they are in input.dtype or float32 and their
    gradients come back in that dtype; grad_weight is the kernel's fp32 buffer cast to weight.dtype (unrounded for an fp32 weight)."""
    B, H, W, C, Cout, Ho, Wo, kh, kw = g[:9]
    dt, dev, K = input.dtype, input.device, g[7] * g[8]
    x = _nhwc_16bit(input)
    dy0 = _nhwc_16bit(grad_output if grad_output.dtype == dt else grad_output.to(dt)).view(B * Ho * Wo, Cout)
    wt = _wt(weight if weight.dtype == dt else weight.to(dt))
    dy = dy0
    pad = (-Cout) % 8            # the kernels read output channels eight at a time: pad with zero columns
    if pad:
        dy = torch.nn.functional.pad(dy0, (0, pad))
        wt = torch.nn.functional.pad(wt, (0, pad))
        g = g[:4] + (Cout + pad,) + g[5:]
    om = offset.dtype if offset.dtype == mask.dtype and offset.dtype in (dt, torch.float32) else torch.float32
    off = (offset if offset.dtype == om else offset.to(om)).contiguous()
    msk = (mask if mask.dtype == om else mask.to(om)).contiguous()
    dx = torch.empty((B, H, W, C), dtype=dt, device=dev)
    doff, dmask = torch.empty_like(off), torch.empty_like(msk)
    dwt = torch.empty((K, C, Cout + pad), dtype=torch.float32, device=dev)
    with _nat.device_guard(dev):
        nb = _nat.lib().fv2p_dcn_backward_h_ws_bytes(B, H, W, Ho, Wo, C, Cout + pad, kh, kw, g[15])
        ws = _nat.workspace(nb, dev)
        _nat.call("fv2p_dcn_backward_h", x, wt, off, msk, dy, *g, dx, doff, dmask, dwt, ws, ws.numel(), _DT16[dt],
                  0 if om == torch.float32 else _DT16[dt], _nat.stream())
        if _channels_last(input) or dx.numel() == 0:
            grad_input = dx.permute(0, 3, 1, 2) if _channels_last(input) else dx.permute(0, 3, 1, 2).contiguous()
        else:
            grad_input = torch.empty((B, C, H, W), dtype=dt, device=dev)
            _nat.call("fv2p_transpose_batched_h", dx, B, H * W, C, grad_input, _nat.stream())
    grad_weight = dwt[:, :, :Cout].reshape(kh, kw, C, Cout).permute(3, 2, 0, 1).contiguous().to(weight.dtype)
    grad_bias = dy0.sum(dim=0, dtype=torch.float32)
    return [grad_input, doff, dmask, grad_weight, grad_bias]


def _forward_nhwc(x, weight, bias, offset, mask, g):
    """x NHWC contiguous fp32 -> y [B*Ho*Wo, Cout] (the C-ABI call)."""
    B, H, W, C, Cout, Ho, Wo = g[:7]
    y = torch.empty((B * Ho * Wo, Cout), dtype=torch.float32, device=x.device)
    with _nat.device_guard(x.device):
        _nat.call("fv2p_dcn_forward", x, _wt_oc(weight.float()), bias.float().contiguous() if bias is not None else None,
                  offset.float().contiguous(), mask.float().contiguous(), *g, y, _nat.stream())
    return y


def _grouped_forward(input, weight, bias, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
                     group, deformable_group):
    """fv2p_dcn_forward_grouped on the padded channels: x [B,H,W,Cin'] and wt_oc [K][Cout][Cin'/G] with zero channels in every piece."""
    g, tail = _geom_grouped(input, weight, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
                            deformable_group)
    B, H, W, Cp, Cout, Ho, Wo = g[:7]
    x = _tail_pad(_to_nhwc(input), tail)
    wt_oc = _tail_pad(weight.float().permute(2, 3, 0, 1), tail).reshape(kernel_h * kernel_w, Cout, Cp // group).contiguous()
    y = torch.empty((B * Ho * Wo, Cout), dtype=torch.float32, device=x.device)
    with _nat.device_guard(x.device):
        _nat.call("fv2p_dcn_forward_grouped", x, wt_oc, bias.float().contiguous() if bias is not None else None,
                  offset.float().contiguous(), mask.float().contiguous(), *g, group, y, _nat.stream())
    y = y.view(B, Ho, Wo, Cout)
    if _channels_last(input):
        return y.permute(0, 3, 1, 2).to(input.dtype)
    return _to_nchw(y).to(input.dtype)


def _grouped_backward(input, weight, offset, mask, grad_output, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h,
                      dilation_w, group, deformable_group):
    """fv2p_dcn_backward_grouped on the padded channels; each group's output columns padded to a multiple of 4 with zeros (in dy and
    the weight), grad_input and grad_weight sliced back to the real channels."""
    g, tail = _geom_grouped(input, weight, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
                            deformable_group)
    B, H, W, Cp, Cout, Ho, Wo = g[:7]
    K, C, dev = kernel_h * kernel_w, input.shape[1], input.device
    cing, coutg = Cp // group, Cout // group
    cop = coutg + (-coutg) % 4      # the kernels read output channels four at a time
    x = _tail_pad(_to_nhwc(input), tail)
    dy0 = _to_nhwc(grad_output).view(B * Ho * Wo, Cout)
    dy = dy0
    if cop != coutg:
        dy = torch.nn.functional.pad(dy0.view(-1, group, coutg), (0, cop - coutg)).reshape(-1, group * cop)
    # [Cout, Cin/G, kh, kw] -> [K][Cin'][Cout'/G]: wt[k][g*cing + c][o] = W[g*coutg + o, c, k]
    w = _tail_pad(weight.float().permute(0, 2, 3, 1), tail)                        # [Cout, kh, kw, cing]
    wz = w.new_zeros((group, cop, kernel_h, kernel_w, cing))
    wz[:, :coutg] = w.reshape(group, coutg, kernel_h, kernel_w, cing)
    wt = wz.permute(2, 3, 0, 4, 1).reshape(K, Cp, cop).contiguous()
    g = g[:4] + (group * cop,) + g[5:]
    dx = torch.empty_like(x)
    doff = torch.empty_like(offset, dtype=torch.float32).contiguous()
    dmask = torch.empty_like(mask, dtype=torch.float32).contiguous()
    dwt = torch.empty((K, Cp, cop), dtype=torch.float32, device=dev)
    with _nat.device_guard(dev):
        nb = _nat.lib().fv2p_dcn_backward_grouped_ws_bytes(B, H, W, Ho, Wo, Cp, group * cop, kernel_h, kernel_w, deformable_group, group)
        ws = _nat.workspace(nb, dev)
        _nat.call("fv2p_dcn_backward_grouped", x, wt, offset.float().contiguous(), mask.float().contiguous(), dy, *g, group, dx, doff,
                  dmask, dwt, ws, ws.numel(), _nat.stream())
    dx = _tail_unpad(dx, tail)
    grad_input = dx.permute(0, 3, 1, 2) if _channels_last(input) else _to_nchw(dx)
    dw = _tail_unpad(dwt.view(K, group, cing, cop)[..., :coutg].transpose(2, 3), tail)     # [K, G, coutg, Cin/G]
    grad_weight = dw.permute(1, 2, 3, 0).reshape(Cout, C // group, kernel_h, kernel_w).contiguous()
    grad_bias = dy0.sum(dim=0)
    return [grad_input, doff, dmask, grad_weight, grad_bias]


def modulated_deform_conv_forward(input, weight, bias, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                                  dilation_h, dilation_w, group, deformable_group, im2col_step):
    """-> output [B, Cout, Ho, Wo] (contiguous NCHW, as modulated_deform_conv_cuda.cu:118). im2col_step is accepted and
    irrelevant: the forward has no columns buffer to chunk.  A channels-last `input` is taken as it is and the output is channels-last
    too (the kernels' own layout: no copy on either side); grad_input follows the input's format likewise."""
    if _native_16bit(input, weight, group, deformable_group):
        g = _geom(input, weight, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, deformable_group)
        return _forward_16bit(input, weight, bias, offset, mask, g)
    if not _plain(input, weight, group, deformable_group):
        return _grouped_forward(input, weight, bias, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h,
                                dilation_w, group, deformable_group)
    g = _geom(input, weight, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, deformable_group)
    B, H, W, C, Cout, Ho, Wo = g[:7]
    x = _to_nhwc(input)
    y = _forward_nhwc(x, weight, bias, offset, mask, g).view(B, Ho, Wo, Cout)
    if _channels_last(input):   # as torch's own ops: a channels-last input gets a channels-last output (here: the kernel's layout, no copy)
        return y.permute(0, 3, 1, 2).to(input.dtype)
    return _to_nchw(y).to(input.dtype)


def modulated_deform_conv_backward(input, weight, bias, offset, mask, grad_output, kernel_h, kernel_w, stride_h, stride_w, pad_h,
                                   pad_w, dilation_h, dilation_w, group, deformable_group, im2col_step):
    """-> [grad_input, grad_offset, grad_mask, grad_weight, grad_bias] (modulated_deform_conv_cuda.cu:127-280).
    No float atomics anywhere: the five gradients are bit-identical from run to run (include/fv2p_ops.h, A13)."""
    if _native_16bit_backward(input, weight, group, deformable_group):
        g = _geom(input, weight, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, deformable_group)
        return _backward_16bit(input, weight, offset, mask, grad_output, g)
    if not _plain(input, weight, group, deformable_group):
        return _grouped_backward(input, weight, offset, mask, grad_output, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                                 dilation_h, dilation_w, group, deformable_group)
    g = _geom(input, weight, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, deformable_group)
    B, H, W, C, Cout, Ho, Wo = g[:7]
    dev = input.device
    x = _to_nhwc_f32(input)
    dy = _to_nhwc_f32(grad_output).view(B * Ho * Wo, Cout)
    wt = _wt(weight.float())
    pad = (-Cout) % 4            # the kernels read output channels four at a time: pad with zero columns
    if pad:
        dy = torch.nn.functional.pad(dy, (0, pad))
        wt = torch.nn.functional.pad(wt, (0, pad))
        g = g[:4] + (Cout + pad,) + g[5:]
    dx = torch.empty_like(x)
    doff = torch.empty_like(offset, dtype=torch.float32).contiguous()
    dmask = torch.empty_like(mask, dtype=torch.float32).contiguous()
    dwt = torch.empty((kernel_h * kernel_w, C, Cout + pad), dtype=torch.float32, device=dev)
    with _nat.device_guard(dev):
        nb = _nat.lib().fv2p_dcn_backward_ws_bytes(B, H, W, Ho, Wo, C, Cout + pad, kernel_h, kernel_w, deformable_group)
        ws = _nat.workspace(nb, dev)
        _nat.call("fv2p_dcn_backward", x, wt, offset.float().contiguous(), mask.float().contiguous(), dy, *g, dx, doff,
                  dmask, dwt, ws, ws.numel(), _nat.stream())
    grad_input = dx.permute(0, 3, 1, 2) if _channels_last(input) else _to_nchw_as(dx, input.dtype if input.dtype in _DT16 else dx.dtype)
    grad_weight = dwt[:, :, :Cout].reshape(kernel_h, kernel_w, C, Cout).permute(3, 2, 0, 1).contiguous()
    grad_bias = dy[:, :Cout].sum(dim=0)
    return [grad_input, doff, dmask, grad_weight, grad_bias]


def deform_conv_forward(input, weight, bias, offset, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
                        group, deformable_group, im2col_step):
    """DCNv1 = DCNv2 with an all-ones modulation mask (deform_im2col_cuda.cuh:127-190 vs modulated_*:127-194)."""
    B, _, Ho, Wo = offset.shape
    mask = torch.ones((B, deformable_group * kernel_h * kernel_w, Ho, Wo), device=input.device,
                      dtype=input.dtype if _native_16bit(input, weight, group, deformable_group) else torch.float32)
    return modulated_deform_conv_forward(input, weight, bias, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                                         dilation_h, dilation_w, group, deformable_group, im2col_step)


def deform_conv_backward(input, weight, bias, offset, grad_output, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h,
                         dilation_w, group, deformable_group, im2col_step):
    """-> [grad_input, grad_offset, grad_weight, grad_bias]."""
    B, _, Ho, Wo = offset.shape
    mask = torch.ones((B, deformable_group * kernel_h * kernel_w, Ho, Wo), device=input.device,
                      dtype=input.dtype if _native_16bit_backward(input, weight, group, deformable_group) else torch.float32)
    gi, go, _, gw, gb = modulated_deform_conv_backward(input, weight, bias, offset, mask, grad_output, kernel_h, kernel_w, stride_h,
                                                       stride_w, pad_h, pad_w, dilation_h, dilation_w, group, deformable_group,
                                                       im2col_step)
    return [gi, go, gw, gb]


def _ps_geom(input, bbox, trans, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size, sample_per_part, trans_std):
    _nat.require_cuda(input, bbox, *(() if no_trans else (trans,)))  # as the reference dispatcher (deform_psroi_pooling.h: "Not implemented on the CPU")
    B, C, H, W = input.shape
    assert C == output_dim, "input channels and output channels must equal"   # deform_psroi_pooling_cuda.cu:291
    classes = 1 if no_trans else trans.shape[1] // 2
    return (B, C, H, W, bbox.shape[0], int(no_trans), float(spatial_scale), output_dim, group_size, pooled_size, part_size,
            sample_per_part, float(trans_std), classes)


def deform_psroi_pooling_forward(input, bbox, trans, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size,
                                 sample_per_part, trans_std):
    """-> (output, top_count), both [num_rois, output_dim, pooled, pooled] (deform_psroi_pooling_cuda.cu:264-341).
    bbox [num_rois, 5] = (batch index, x1, y1, x2, y2); trans [>= num_rois, 2 * num_classes, part, part] (ignored with no_trans)."""
    g = _ps_geom(input, bbox, trans, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size, sample_per_part, trans_std)
    x = input.float().contiguous()
    out = torch.empty((bbox.shape[0], output_dim, pooled_size, pooled_size), dtype=torch.float32, device=input.device)
    top_count = torch.zeros_like(out)
    with _nat.device_guard(input.device):
        _nat.call("fv2p_deform_psroi_pool_forward", x, bbox.float().contiguous(), None if no_trans else trans.float().contiguous(), *g,
                  out, top_count, _nat.stream())
    return out.to(input.dtype), top_count.to(input.dtype)


def deform_psroi_pooling_backward(out_grad, input, bbox, trans, top_count, no_trans, spatial_scale, output_dim, group_size, pooled_size,
                                  part_size, sample_per_part, trans_std):
    """-> (input_grad, trans_grad) (deform_psroi_pooling_cuda.cu:343-418); trans_grad has trans's shape."""
    g = _ps_geom(input, bbox, trans, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size, sample_per_part, trans_std)
    x = input.float().contiguous()
    dx = torch.zeros_like(x)
    dtrans = torch.zeros_like(trans, dtype=torch.float32).contiguous()
    if _nat.deterministic():   # fixed-order form (fv2p_scatter_add): writes dx and dtrans's first len(bbox) rows
        with _nat.device_guard(input.device):
            ws = _nat.workspace(_nat.lib().fv2p_deform_psroi_pool_backward_ws_bytes(g[4], g[7], g[9], g[11]), input.device)
            _nat.call("fv2p_deform_psroi_pool_backward_gather", out_grad.float().contiguous(), x, bbox.float().contiguous(),
                      None if no_trans else trans.float().contiguous(), top_count.float().contiguous(), *g, dx,
                      None if no_trans else dtrans, ws, ws.numel(), _nat.stream())
        return dx.to(input.dtype), dtrans.to(trans.dtype)
    with _nat.device_guard(input.device):
        _nat.call("fv2p_deform_psroi_pool_backward", out_grad.float().contiguous(), x, bbox.float().contiguous(),
                  None if no_trans else trans.float().contiguous(), top_count.float().contiguous(), *g, dx,
                  None if no_trans else dtrans, _nat.stream())
    return dx.to(input.dtype), dtrans.to(trans.dtype)
