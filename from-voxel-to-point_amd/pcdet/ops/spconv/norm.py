"""BatchNorm1d (+ReLU) on sparse-tensor features as two HIP launches forward and two backward.

The reference builds every backbone block as ``SparseSequential(conv, nn.BatchNorm1d(eps=1e-3, momentum=0.01),
nn.ReLU())`` (pcdet/models/backbones_3d/spconv_backbone.py:8-27, :75) and ``SparseSequential.forward`` applies the two
torch modules to ``.features`` (pcdet/ops/spconv/modules.py:86-100).  ``batch_norm_relu`` is what this package's
``SparseSequential`` calls for that pair instead: same parameters, same running-statistics update, same result within
fp32 rounding, kernels in csrc/batchnorm.hip.  It returns None whenever the situation is not the plain one (hooks on
the modules, autocast, CPU tensors, a single row in training mode ...) and the caller then runs the torch
modules one by one, so error behaviour stays torch's.  (`spconv.set_mixed_precision(True)` lifts the autocast rule for the 16-bit
route below, and for it alone.)

float16 / bfloat16 features take a route of their own (`fusable16`, `_BatchNormReLU16`, the Fmt16 instances of the kernels in csrc/batchnorm.hip): x, y and
the gradients stay in 16 bits, the arithmetic is fp32 with one rounding at the store, and the module's parameters and buffers are
either all fp32 or all of x's dtype.  Nothing is cast on the way.  That route also takes the `residual` of a residual block's tail,
y = relu(bn(x) + residual).

Dense maps [N, C, H, W] have the same op for `nn.BatchNorm2d` (`fusable2d`, `batch_norm2d_relu`, `run_maps`; kernels in
csrc/batchnorm2d.hip): at the end of this file.  float16 / bfloat16 maps take `fusable2d16`, `batch_norm2d_relu16` and the same kernels
in their format, by the rules of the 16-bit row route; `run_maps` tries them where the fp32 op declined.
"""
import os

import torch
from torch import nn
from torch.autograd import Function

import fv2p_native as _nat

from . import ops as _ops
from .._glue import DT16 as _DT16

_ENABLED = os.environ.get("FV2P_FUSED_BN", "1") != "0"


_WS_BYTES = {}


def _ws_bytes(c):
    b = _WS_BYTES.get(c)
    if b is None:
        b = _WS_BYTES[c] = _nat.call("fv2p_batchnorm_ws_bytes", 0, c)
    return b


class _BatchNormReLU(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, bn, relu):
        n, c = x.shape
        dev = x.device
        batch_stats = bn.training or bn.running_mean is None
        y = torch.empty_like(x)
        with _nat.device_guard(dev):
            if batch_stats:
                stats = torch.empty((2, c), dtype=torch.float32, device=dev)
                mean, invstd = stats[0], stats[1]
                track = bn.training and bn.running_mean is not None
                ws = _nat.workspace(_ws_bytes(c), dev)
                _nat.call("fv2p_batchnorm_forward", x, n, c, float(bn.eps), -1.0 if bn.momentum is None else float(bn.momentum),
                          weight, bias, int(relu), bn.running_mean if track else None, bn.running_var if track else None,
                          bn.num_batches_tracked if track else None, mean, invstd, y, ws, ws.numel(), _nat.stream())
            else:
                mean = bn.running_mean
                invstd = torch.rsqrt(bn.running_var + bn.eps)
                _nat.call("fv2p_batchnorm_apply", x, n, c, mean, invstd, weight, bias, int(relu), y, _nat.stream())
        ctx.save_for_backward(x, mean, invstd, weight, bias)
        ctx.relu, ctx.batch_stats = bool(relu), bool(batch_stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, invstd, weight, bias = ctx.saved_tensors
        n, c = x.shape
        dev = x.device
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dpar = torch.empty((2, c), dtype=torch.float32, device=dev)
        dgamma, dbeta = dpar[0], dpar[1]
        with _nat.device_guard(dev):
            ws = _nat.workspace(_ws_bytes(c), dev)
            _nat.call("fv2p_batchnorm_backward", x, dy, n, c, mean, invstd, weight, bias, int(ctx.relu), int(ctx.batch_stats),
                      dx, dgamma, dbeta, ws, ws.numel(), _nat.stream())
        return (dx if ctx.needs_input_grad[0] else None, dgamma if (weight is not None and ctx.needs_input_grad[1]) else None,
                dbeta if (bias is not None and ctx.needs_input_grad[2]) else None, None, None)


_WS_BYTES16 = {}


def _ws_bytes16(c):
    b = _WS_BYTES16.get(c)
    if b is None:
        b = _WS_BYTES16[c] = _nat.call("fv2p_batchnorm_h_ws_bytes", 0, c)
    return b


class _BatchNormReLU16(Function):
    """y = relu?(bn(x) [+ residual]) on float16 / bfloat16 rows.  Saves x, the fp32 mean / invstd and the parameters (and y in the
    residual form, whose ReLU mask cannot be recomputed from x alone)."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, bn, relu):
        n, c = x.shape
        dev = x.device
        dt = _DT16[x.dtype]
        pd = 0 if _param_dtype(bn) in (None, torch.float32) else dt
        batch_stats = bn.training or bn.running_mean is None
        y = torch.empty_like(x)
        with _nat.device_guard(dev):
            if batch_stats:
                stats = torch.empty((2, c), dtype=torch.float32, device=dev)
                mean, invstd = stats[0], stats[1]
                track = bn.training and bn.running_mean is not None
                ws = _nat.workspace(_ws_bytes16(c), dev)
                _nat.call("fv2p_batchnorm_forward_h", x, n, c, float(bn.eps), -1.0 if bn.momentum is None else float(bn.momentum),
                          weight, bias, int(relu), residual, bn.running_mean if track else None, bn.running_var if track else None,
                          bn.num_batches_tracked if track else None, mean, invstd, y, dt, pd, ws, ws.numel(), _nat.stream())
            else:
                # [C] values: widened here, 1 / sqrt in float64 so that invstd is the correctly rounded fp32 value
                mean = bn.running_mean.float()
                invstd = (1.0 / torch.sqrt(bn.running_var.double() + bn.eps)).float()
                _nat.call("fv2p_batchnorm_apply_h", x, n, c, mean, invstd, weight, bias, int(relu), residual, y, dt, pd, _nat.stream())
        mask_y = y if (residual is not None and relu) else None
        ctx.save_for_backward(x, mean, invstd, weight, bias, mask_y)
        ctx.relu, ctx.batch_stats, ctx.dt, ctx.pd, ctx.has_res = bool(relu), bool(batch_stats), dt, pd, residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, invstd, weight, bias, mask_y = ctx.saved_tensors
        n, c = x.shape
        dev = x.device
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        # the identity branch's gradient: dy * [y > 0] with a ReLU, dy itself without
        dres = torch.empty_like(x) if (ctx.has_res and ctx.relu and ctx.needs_input_grad[3]) else None
        dpar = torch.empty((2, c), dtype=x.dtype if ctx.pd else torch.float32, device=dev)
        dgamma, dbeta = dpar[0], dpar[1]
        with _nat.device_guard(dev):
            ws = _nat.workspace(_ws_bytes16(c), dev)
            _nat.call("fv2p_batchnorm_backward_h", x, dy, n, c, mean, invstd, weight, bias, int(ctx.relu), int(ctx.batch_stats), mask_y,
                      dx, dres, dgamma, dbeta, ctx.dt, ctx.pd, ws, ws.numel(), _nat.stream())
        if ctx.has_res and not ctx.relu and ctx.needs_input_grad[3]:
            dres = dy
        return (dx if ctx.needs_input_grad[0] else None, dgamma if (weight is not None and ctx.needs_input_grad[1]) else None,
                dbeta if (bias is not None and ctx.needs_input_grad[2]) else None, dres, None, None)


def _plain(module):
    return not (module._forward_hooks or module._forward_pre_hooks or module._backward_hooks)


def _param_dtype(bn):
    """The one dtype of bn's floating parameters and buffers, None when it has none, False when they are mixed or not on the GPU."""
    ts = [t for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var) if t is not None]
    if any(not t.is_cuda for t in ts) or len({t.dtype for t in ts}) > 1:
        return False
    return ts[0].dtype if ts else None


def fusable16(bn, relu_module, x, channels):
    """The plain case of the (BatchNorm1d, ReLU) pair on float16 / bfloat16 features x [N, channels] the 16-bit op covers."""
    if not _ENABLED or type(bn) is not nn.BatchNorm1d or not _plain(bn):
        return False
    if relu_module is not None and (type(relu_module) is not nn.ReLU or not _plain(relu_module)):
        return False
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype in _DT16 and x.dim() == 2 and x.is_contiguous()):
        return False
    if torch.is_autocast_enabled() and not _ops.mixed_precision():   # (mixed precision: 16-bit rows under autocast are this route's case)
        return False
    if channels != bn.num_features or x.shape[1] != channels:
        return False
    c = channels
    if c > 256 and c % 8 != 0 or c > 1024:
        return False
    if (bn.weight is None) != (bn.bias is None):
        return False
    pdt = _param_dtype(bn)
    if pdt is False or pdt not in (None, torch.float32, x.dtype):
        return False
    if bn.training and x.shape[0] < 2:
        return False
    return True


def fusable(bn, relu_module, x, channels):
    """The plain case of the (BatchNorm1d, ReLU) pair on features x [N, channels] the fused op covers."""
    if not _ENABLED or type(bn) is not nn.BatchNorm1d or not _plain(bn):
        return False
    if relu_module is not None and (type(relu_module) is not nn.ReLU or not _plain(relu_module)):
        return False
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2):
        return False
    if torch.is_autocast_enabled() or channels != bn.num_features:
        return False
    c = channels
    if c > 256 and c % 4 != 0 or c > 1024:
        return False
    if bn.weight is not None and (bn.weight.dtype != torch.float32 or not bn.weight.is_cuda):
        return False
    return True


def batch_norm_relu(bn, x, relu_module=None, residual=None):
    """y = relu?(bn(x)) for x [N, C] on the GPU, or None when the fused path does not apply.  float16 / bfloat16 x runs the 16-bit
    kernels and may bring a `residual` of x's shape and dtype: y = relu?(bn(x) + residual).  (fp32 x with a residual: None.)"""
    if torch.is_tensor(x) and x.dtype in _DT16:
        if x.dim() != 2 or not fusable16(bn, relu_module, x, x.shape[1]) or x.shape[0] == 0:
            return None
        if residual is not None:
            if not (torch.is_tensor(residual) and residual.is_cuda and residual.dtype == x.dtype and residual.shape == x.shape):
                return None
            residual = residual.contiguous()
        return _BatchNormReLU16.apply(x, bn.weight, bn.bias, residual, bn, relu_module is not None)
    if residual is not None:
        return None
    if not (torch.is_tensor(x) and x.dim() == 2 and x.is_contiguous() and fusable(bn, relu_module, x, x.shape[1])):
        return None
    if x.shape[0] < 2:
        return None
    ext = _nat.torch_ext()
    if ext is not None:
        return ext.batch_norm_relu(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.training,
                                   -1.0 if bn.momentum is None else float(bn.momentum), float(bn.eps), relu_module is not None)
    return _BatchNormReLU.apply(x, bn.weight, bn.bias, bn, relu_module is not None)


# ---- BatchNorm2d (+ReLU) on contiguous NCHW maps (csrc/batchnorm2d.hip) ---------------------------------------------------------------
# The pair behind every Conv2d / ConvTranspose2d of the BEV backbones (base_bev_backbone.py:35-46, :53-70).  Same contract as the row op
# above: the module's parameters and running statistics, torch's result within fp32 rounding, None whenever the situation is not the
# plain one - and the caller then runs the torch modules one by one.
# float16 / bfloat16 maps run the same kernels in their format: x, y and the gradients stay in 16 bits; fp32 arithmetic, fp64 sums, one
# rounding at the store; the module's parameters and buffers are all fp32 (a BatchNorm kept in fp32 under autocast) or all of x's dtype
# (backbone_2d.half()).  Nothing is cast on the way.
BN2D_CHUNK = 4096   # plane elements per workgroup (kBn2dChunk in csrc/batchnorm2d.hip); tests place shapes on either side of it
BN2D_CHUNK16 = BN2D_CHUNK   # the same kernels, the same chunk
_WS_BYTES2D = {}


def _ws_bytes2d(n, c, hw):
    b = _WS_BYTES2D.get((n, c, hw))
    if b is None:
        b = _WS_BYTES2D[(n, c, hw)] = _nat.call("fv2p_batchnorm2d_ws_bytes", n, c, hw)   # (the _h query returns the same)
    return b


class _BatchNorm2dReLU(Function):
    """y = relu?(bn(x)) on an fp32, float16 or bfloat16 map.  Saves x, the fp32 mean / invstd and the parameters; the backward pass
    recomputes the mask of the stored y from x.  (fp32 maps: the ctypes form of the compiled binding's BnRelu2dFn, used when
    lib/fv2p_torch.so is absent.)"""

    @staticmethod
    def forward(ctx, x, weight, bias, bn, relu):
        n, c, h, w = x.shape
        hw = h * w
        dev = x.device
        # the 16-bit entry points (`_h`) take the map's format and the parameters' after the outputs; the fp32 ones take neither
        if x.dtype in _DT16:
            dt = _DT16[x.dtype]
            pd = 0 if _param_dtype(bn) in (None, torch.float32) else dt
            sfx, fmt = "_h", (dt, pd)
        else:
            pd, sfx, fmt = 0, "", ()
        batch_stats = bn.training or bn.running_mean is None
        y = torch.empty_like(x)
        with _nat.device_guard(dev):
            if batch_stats:
                stats = torch.empty((2, c), dtype=torch.float32, device=dev)
                mean, invstd = stats[0], stats[1]
                track = bn.training and bn.running_mean is not None
                ws = _nat.workspace(_ws_bytes2d(n, c, hw), dev)
                _nat.call("fv2p_batchnorm2d_forward" + sfx, x, n, c, hw, float(bn.eps), -1.0 if bn.momentum is None else float(bn.momentum),
                          weight, bias, int(relu), bn.running_mean if track else None, bn.running_var if track else None,
                          bn.num_batches_tracked if track else None, mean, invstd, y, *fmt, ws, ws.numel(), _nat.stream())
            else:
                # [C] values.  mean is a copy: the buffer may move before this call's backward runs.  The two formats keep their own
                # invstd because the bits differ: fp32 maps take torch's fp32 rsqrt (what the compiled binding computes), 16-bit maps
                # widen the buffers and take 1 / sqrt in float64, so that invstd is the correctly rounded fp32 value
                if fmt:
                    mean = bn.running_mean.float().clone()
                    invstd = (1.0 / torch.sqrt(bn.running_var.double() + bn.eps)).float()
                else:
                    mean = bn.running_mean.clone()
                    invstd = torch.rsqrt(bn.running_var + bn.eps)
                _nat.call("fv2p_batchnorm2d_apply" + sfx, x, n, c, hw, mean, invstd, weight, bias, int(relu), y, *fmt, _nat.stream())
        ctx.save_for_backward(x, mean, invstd, weight, bias)
        ctx.relu, ctx.batch_stats, ctx.pd, ctx.sfx, ctx.fmt = bool(relu), bool(batch_stats), pd, sfx, fmt
        return y

    @staticmethod
    def backward(ctx, dz):
        x, mean, invstd, weight, bias = ctx.saved_tensors
        n, c, h, w = x.shape
        hw = h * w
        dev = x.device
        dz = dz.contiguous()
        dx = torch.empty_like(x)
        dpar = torch.empty((2, c), dtype=x.dtype if ctx.pd else torch.float32, device=dev)
        dgamma, dbeta = dpar[0], dpar[1]
        with _nat.device_guard(dev):
            ws = _nat.workspace(_ws_bytes2d(n, c, hw), dev)
            _nat.call("fv2p_batchnorm2d_backward" + ctx.sfx, x, dz, n, c, hw, mean, invstd, weight, bias, int(ctx.relu), int(ctx.batch_stats),
                      dx, dgamma, dbeta, *ctx.fmt, ws, ws.numel(), _nat.stream())
        return (dx if ctx.needs_input_grad[0] else None, dgamma if (weight is not None and ctx.needs_input_grad[1]) else None,
                dbeta if (bias is not None and ctx.needs_input_grad[2]) else None, None, None)


class _BatchNorm2dReLU16(_BatchNorm2dReLU):
    """The same Function under the name a 16-bit map's grad_fn shows (`_BatchNorm2dReLU16Backward`): what says that no fp32 op ran."""


def _plain_forward(module):
    """No hooks, and `forward` is the class's own (not replaced on the instance)."""
    return _plain(module) and "forward" not in module.__dict__


def _fusable2d(bn, relu_module, x, dtypes, autocast_ok, params_ok):
    """The plain case of the (BatchNorm2d, ReLU) pair on a map x [N, C, H, W] of one of `dtypes`.  The two routes differ in what they
    accept under autocast (`autocast_ok()`) and in the dtypes of the module's parameters and buffers (`params_ok(bn, x)`)."""
    if not _ENABLED or type(bn) is not nn.BatchNorm2d or not _plain_forward(bn):
        return False
    if relu_module is not None and (type(relu_module) is not nn.ReLU or not _plain_forward(relu_module)):
        return False
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype in dtypes and x.dim() == 4):
        return False
    if not x.is_contiguous() or x.shape[1] != bn.num_features:   # (channels_last maps are not NCHW-contiguous: torch's modules run)
        return False
    if torch.is_autocast_enabled() and not autocast_ok():
        return False
    n, _, h, w = x.shape
    if n * h * w < (2 if bn.training else 1):   # torch raises for a single value per channel in training mode: let it
        return False
    if (bn.weight is None) != (bn.bias is None):
        return False
    if not params_ok(bn, x):
        return False
    for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked):
        if t is not None and t.device != x.device:
            return False
    return True


def _params_fp32(bn, x):
    return all(t is None or t.dtype == torch.float32 for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))


def _params_fp32_or_x(bn, x):
    pdt = _param_dtype(bn)   # (False: mixed, or not on the GPU)
    return pdt is not False and pdt in (None, torch.float32, x.dtype)


def fusable2d(bn, relu_module, x):
    """The plain case of the (BatchNorm2d, ReLU) pair on an fp32 map x [N, C, H, W] the fused op covers: never under autocast, fp32
    parameters."""
    return _fusable2d(bn, relu_module, x, (torch.float32,), lambda: False, _params_fp32)


def fusable2d16(bn, relu_module, x):
    """The plain case of the (BatchNorm2d, ReLU) pair on a float16 / bfloat16 map x [N, C, H, W] the 16-bit op covers: under autocast
    only in mixed precision (the rule of fusable16), parameters all fp32 or all of x's dtype."""
    return _fusable2d(bn, relu_module, x, _DT16, _ops.mixed_precision, _params_fp32_or_x)


def batch_norm2d_relu(bn, x, relu_module=None):
    """y = relu?(bn(x)) for a contiguous fp32 map x [N, C, H, W] on the GPU, or None when the fused path does not apply."""
    if not fusable2d(bn, relu_module, x):
        return None
    ext = _nat.torch_ext()
    if ext is not None:
        return ext.batch_norm2d_relu(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.training,
                                     -1.0 if bn.momentum is None else float(bn.momentum), float(bn.eps), relu_module is not None)
    return _BatchNorm2dReLU.apply(x, bn.weight, bn.bias, bn, relu_module is not None)


def batch_norm2d_relu16(bn, x, relu_module=None):
    """y = relu?(bn(x)) for a contiguous float16 / bfloat16 map x [N, C, H, W] on the GPU, in x's dtype, or None when the 16-bit path
    does not apply."""
    if not fusable2d16(bn, relu_module, x):
        return None
    return _BatchNorm2dReLU16.apply(x, bn.weight, bn.bias, bn, relu_module is not None)


def _bn2d_either(bn, x, relu_module):
    y = batch_norm2d_relu(bn, x, relu_module)
    return y if y is not None else batch_norm2d_relu16(bn, x, relu_module)


def run_maps(mods, x):
    """The modules `mods` (a Sequential of Conv2d / ConvTranspose2d / BatchNorm2d / ReLU / ...) applied to the map x in order, with every
    (BatchNorm2d, ReLU) pair - or a BatchNorm2d alone - the fused op covers as one call.  Anything else runs as the module itself."""
    mods = list(mods)
    i = 0
    while i < len(mods):
        m = mods[i]
        if type(m) is nn.BatchNorm2d:
            relu = mods[i + 1] if i + 1 < len(mods) and type(mods[i + 1]) is nn.ReLU else None
            y = _bn2d_either(m, x, relu)     # the fp32 op, the 16-bit op where it declined
            if y is None and relu is not None:   # the ReLU module is not a plain one: the BatchNorm alone, then the module
                relu = None
                y = _bn2d_either(m, x, None)
            if y is not None:
                x = y
                i += 1 + (relu is not None)
                continue
        x = m(x)
        i += 1
    return x
