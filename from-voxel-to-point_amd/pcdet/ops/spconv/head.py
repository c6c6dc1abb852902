"""The 1x1 convolutions of a dense head as one op on the BEV map (kernels in csrc/head1x1.hip).

The reference's anchor head runs three independent ``nn.Conv2d(cin, c_k, kernel_size=1)`` over the same map and permutes every
output to position-major (pcdet/models/dense_heads/anchor_head_single.py:21-37, :48-60).  ``multi_conv1x1`` is what the harness
calls for those modules instead: the map is read once forward, its gradient is written once, the weight and bias gradients come
from one more read, and the outputs arrive as ``[B, H * W, c_k]`` - the layout ``conv(x).permute(0, 2, 3, 1).reshape(b, -1, c_k)``
followed by ``.contiguous()`` has.  Same parameters (the modules' own tensors, nothing repacked or cached), torch's result within
fp32 rounding, weight and bias gradients bit-identical from run to run (no atomics: nothing changes under ``set_deterministic``).
It returns None whenever the situation is not the plain one and the caller then runs the modules, so everything else - 16-bit
maps, channels_last maps, autocast, CPU tensors, other kernel sizes, Conv2d subclasses - stays torch's.
"""
import torch
from torch import nn
from torch.autograd import Function

import fv2p_native as _nat

from .norm import _plain_forward

MAX_COLUMNS = 64       # output channels of all heads together (4 MFMA column blocks)
MAX_POSITIONS = 1 << 30
_WS_BYTES = {}


def _ws_bytes(b, cin, hw, cks):
    key = (b, cin, hw, cks)
    v = _WS_BYTES.get(key)
    if v is None:
        v = _WS_BYTES[key] = _nat.call("fv2p_head1x1_ws_bytes", b, cin, hw, *cks)
    return v


def _pad3(seq, fill):
    seq = list(seq)
    return seq + [fill] * (3 - len(seq))


class _Head1x1(Function):
    """(x, w_0, bias_0, w_1, bias_1, ...) -> (y_0, y_1, ...), y_k [B, H * W, c_k]."""

    @staticmethod
    def forward(ctx, x, *params):
        ws, bs = params[0::2], params[1::2]
        b, cin, h, w = x.shape
        hw = h * w
        cks = tuple(int(t.shape[0]) for t in ws)
        ys = [x.new_empty((b, hw, ck)) for ck in cks]
        with _nat.device_guard(x.device):
            _nat.call("fv2p_head1x1_forward", x, b, cin, hw, *_pad3(ws, None), *_pad3(bs, None), *_pad3(cks, 0), *_pad3(ys, None),
                      _nat.stream())
        ctx.save_for_backward(x, *ws)
        ctx.cks, ctx.has_bias = cks, tuple(t is not None for t in bs)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        x, *ws = ctx.saved_tensors
        b, cin, h, w = x.shape
        hw = h * w
        cks = ctx.cks
        dys = [d.contiguous() for d in dys]
        need = ctx.needs_input_grad
        dx = None
        dws, dbs = [None] * len(cks), [None] * len(cks)
        with _nat.device_guard(x.device):
            if need[0]:
                dx = torch.empty_like(x)
                _nat.call("fv2p_head1x1_backward_data", *_pad3(dys, None), b, cin, hw, *_pad3(ws, None), *_pad3(cks, 0), dx, _nat.stream())
            if any(need[1:]):
                dws = [torch.empty_like(t) for t in ws]
                dbs = [x.new_empty(ck) if hb else None for ck, hb in zip(cks, ctx.has_bias)]
                wsp = _nat.workspace(_ws_bytes(b, cin, hw, tuple(_pad3(cks, 0))), x.device)
                _nat.call("fv2p_head1x1_backward_weights", x, *_pad3(dys, None), b, cin, hw, *_pad3(cks, 0), *_pad3(dws, None),
                          *_pad3(dbs, None), wsp, wsp.numel(), _nat.stream())
        grads = [dx]
        for k in range(len(cks)):
            grads.append(dws[k] if need[1 + 2 * k] else None)
            grads.append(dbs[k] if need[2 + 2 * k] else None)
        return tuple(grads)


def _plain_conv1x1(m):
    return (type(m) is nn.Conv2d and _plain_forward(m) and m.kernel_size == (1, 1) and m.stride == (1, 1) and m.padding == (0, 0)
            and m.dilation == (1, 1) and m.groups == 1)


def fusable(mods, x):
    """The plain case the fused op covers: one to three plain nn.Conv2d modules with kernel size 1, stride 1, padding 0, groups 1 and
    at most MAX_COLUMNS output channels together, fp32 parameters, on a contiguous fp32 NCHW map on the GPU, not under autocast."""
    mods = list(mods)
    if not 1 <= len(mods) <= 3 or not all(_plain_conv1x1(m) for m in mods):
        return False
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        return False
    if torch.is_autocast_enabled():
        return False
    b, cin, h, w = x.shape
    if b * h * w < 1 or b * h * w >= MAX_POSITIONS or cin < 1:
        return False
    if sum(m.out_channels for m in mods) > MAX_COLUMNS:
        return False
    for m in mods:
        if m.in_channels != cin:
            return False
        for t in (m.weight, m.bias):
            if t is not None and (t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous()):
                return False
    return True


def multi_conv1x1(mods, x):
    """[conv(x).permute(0, 2, 3, 1).reshape(B, H * W, c_k) for conv in mods], contiguous, from one kernel per direction - or None when
    the fused path does not apply (`fusable`)."""
    mods = list(mods)
    if not fusable(mods, x):
        return None
    params = []
    for m in mods:
        params += [m.weight, m.bias]
    return list(_Head1x1.apply(x, *params))


def run_heads(mods, x):
    """The position-major outputs [B, H * W, c_k] of the conv modules `mods` on the map x: the fused op where it applies, the modules
    themselves (and torch's permute) everywhere else."""
    ys = multi_conv1x1(mods, x)
    if ys is None:
        ys = [m(x).permute(0, 2, 3, 1).reshape(x.shape[0], -1, m.out_channels) for m in mods]
    return ys
