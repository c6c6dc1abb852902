"""nn.Linear(bias=False) -> nn.BatchNorm1d [-> nn.ReLU] on point rows as one op (kernels in csrc/linear_bn.hip: one source for fp32,
float16 and bfloat16 rows).

The voxel-to-point decoder is thirteen such triples over the key-point rows (fv2p_harness/fv2p_model.py: LateralBlock.net /
.downsample, V2PDecoder.decode_block_out) and ``BEVGridPooling.point_bev_feature_compress`` is one more.  ``linear_bn_relu`` is what
their callers try for the three modules instead: the product runs on this library's fp32 MFMA kernels, the BatchNorm statistics come
out of the GEMM's epilogue, and the weight gradient is folded in a fixed order - so the output, every gradient and the running
statistics are bit-identical from run to run without any library determinism setting.  Same parameters (the modules' own tensors,
nothing repacked or cached), the same running-statistics update, torch's result within fp32 rounding.  It returns None whenever the
situation is not the plain one (`fusable`) and the caller then runs the modules, so everything else - a Linear with bias,
autocast, CPU tensors, hooks, subclasses, a single row in training mode - stays torch's, errors included.

16-bit rows: float16 / bfloat16 rows have a route of their own (`fusable16`, `linear_bn_relu16`, `_LinearBatchNormReLU16`: the
same kernels instantiated on the 16-bit MFMA; the two autograd Functions are shells over one forward and one backward body).  x, the pre-activation z, y and every [n, .] gradient stay in 16 bits; z = round(x w^T) as
stored is the pre-activation everywhere (torch's bn(linear(x)) on 16-bit rows); fp32 accumulators, fp64 sums in a fixed order, one
rounding at each store.  The BatchNorm parameters and buffers are all fp32 or all of x's dtype; the Linear weight has x's dtype, or
is an fp32 master weight under autocast with `spconv.set_mixed_precision(True)` (rounded once on its way into LDS, its gradient
fp32).  `fusable` and `linear_bn_relu` keep declining 16-bit rows and autocast: callers ask the 16-bit pair next (`run_rows`).
"""
import os

import torch
from torch import nn
from torch.autograd import Function

import fv2p_native as _nat

from . import ops as _ops
from .norm import _param_dtype, _plain_forward
from .._glue import DT16 as _DT16

_ENABLED = os.environ.get("FV2P_FUSED_LINEAR", "1") != "0"

MAX_IN = 1024     # kMaxCin / kMaxCout of csrc/linear_bn.hip
MAX_OUT = 512


def _asked_once(name):
    """The library's host-side query `name` (workspace bytes, pays) as a function that asks once per argument tuple."""
    memo = {}

    def ask(*args):
        v = memo.get(args)
        if v is None:
            v = memo[args] = _nat.call(name, *args)
        return v
    return ask


_pays = _asked_once("fv2p_linear_bn_pays")
_pays16 = _asked_once("fv2p_linear_bn_h_pays")


def pays(n, cin, cout):
    """Whether the op measured faster than the library route at this shape (fv2p_linear_bn_pays): what `run_rows` and
    BEVGridPooling ask before they use it.  `linear_bn_relu` itself does not ask."""
    return bool(_pays(n, cin, cout))


def pays16(n, cin, cout, dtype):
    """`pays` for the 16-bit op on rows of `dtype` (fv2p_linear_bn_h_pays, cached): measured against the route 16-bit rows take
    without it - the library's product, then the 16-bit BatchNorm op."""
    return bool(_pays16(n, cin, cout, _DT16[dtype]))


def _eval_stats32(bn):
    return bn.running_mean.clone(), torch.rsqrt(bn.running_var + bn.eps)


def _eval_stats16(bn):
    """Widened to fp32; 1 / sqrt in float64 so that invstd is the correctly rounded fp32 value, as _BatchNormReLU16 prepares it (not
    the bits of `_eval_stats32`'s rsqrt)."""
    mean = bn.running_mean.float().clone() if bn.running_mean.dtype == torch.float32 else bn.running_mean.float()
    return mean, (1.0 / torch.sqrt(bn.running_var.double() + bn.eps)).float()


class _Route:
    """What the fp32 rows and the 16-bit rows call: the entry points' names, the workspace query, and eval_stats(bn) -> the fp32
    mean / invstd of a frozen BatchNorm ([cout] copies: the buffers may move before the call's backward runs)."""

    def __init__(self, sfx, eval_stats):
        self.forward, self.forward_eval, self.backward = ("fv2p_linear_bn_%s%s" % (k, sfx) for k in ("forward", "forward_eval", "backward"))
        self.ws_bytes = _asked_once("fv2p_linear_bn%s_ws_bytes" % sfx)
        self.eval_stats = eval_stats


_F32 = _Route("", _eval_stats32)
_H16 = _Route("_h", _eval_stats16)


def _forward(ctx, route, fmt, x, w, gamma, beta, bn, relu, keep_z):
    """The forward pass of both routes; fmt: the trailing (dt, wd, pd) of the _h entry points, () for fp32 rows."""
    n, cin = x.shape
    cout = w.shape[0]
    dev = x.device
    batch_stats = bn.training or bn.running_mean is None
    y = x.new_empty((n, cout))
    with _nat.device_guard(dev):
        if batch_stats:
            z = x.new_empty((n, cout))
            stats = torch.empty((2, cout), dtype=torch.float32, device=dev) if fmt else x.new_empty((2, cout))
            mean, invstd = stats[0], stats[1]
            track = bn.training and bn.running_mean is not None
            ws = _nat.workspace(route.ws_bytes(n, cin, cout), dev)
            _nat.call(route.forward, x, n, cin, w, cout, float(bn.eps), -1.0 if bn.momentum is None else float(bn.momentum),
                      gamma, beta, int(relu), bn.running_mean if track else None, bn.running_var if track else None,
                      bn.num_batches_tracked if track else None, z, mean, invstd, y, *fmt, ws, ws.numel(), _nat.stream())
        else:
            # z is kept only when a gradient can be asked for (the backward pass through the frozen BatchNorm reads it)
            z = x.new_empty((n, cout)) if keep_z else None
            mean, invstd = route.eval_stats(bn)
            _nat.call(route.forward_eval, x, n, cin, w, cout, mean, invstd, gamma, beta, int(relu), z, y, *fmt, _nat.stream())
    ctx.save_for_backward(x, z, mean, invstd, w, gamma, beta)
    ctx.relu, ctx.batch_stats, ctx.route, ctx.fmt = bool(relu), bool(batch_stats), route, fmt
    return y


def _backward(ctx, dy):
    """The backward pass of both routes.  dgamma / dbeta are fp32, or of the rows' dtype where the parameters are (pd)."""
    x, z, mean, invstd, w, gamma, beta = ctx.saved_tensors
    n, cin = x.shape
    cout = w.shape[0]
    dev = x.device
    route, fmt = ctx.route, ctx.fmt
    dy = dy.contiguous()
    need = ctx.needs_input_grad
    du = torch.empty_like(z)
    dx = torch.empty_like(x) if need[0] else None
    dw = torch.empty_like(w) if need[1] else None
    dpar = (mean if fmt and not fmt[2] else x).new_empty((2, cout))
    dgamma, dbeta = dpar[0], dpar[1]
    with _nat.device_guard(dev):
        ws = _nat.workspace(route.ws_bytes(n, cin, cout), dev)
        _nat.call(route.backward, x, z, dy, n, cin, w, cout, mean, invstd, gamma, beta, int(ctx.relu), int(ctx.batch_stats),
                  du, dx, dw, dgamma, dbeta, *fmt, ws, ws.numel(), _nat.stream())
    return (dx, dw, dgamma if (gamma is not None and need[2]) else None, dbeta if (beta is not None and need[3]) else None, None, None, None)


class _LinearBatchNormReLU(Function):
    """(x [n, cin], w [cout, cin], gamma, beta) -> y [n, cout].  Saves x, the pre-activation z, mean / invstd and the parameters; the
    backward pass recomputes the ReLU mask from z."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, bn, relu, keep_z):
        return _forward(ctx, _F32, (), x, w, gamma, beta, bn, relu, keep_z)

    backward = staticmethod(_backward)


class _LinearBatchNormReLU16(Function):
    """(x [n, cin] in T, w [cout, cin] in T or fp32, gamma, beta) -> y [n, cout] in T.  Saves x, the stored 16-bit pre-activation z, the
    fp32 mean / invstd and the parameters; the backward pass recomputes the ReLU mask from z."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, bn, relu, keep_z):
        dt = _DT16[x.dtype]
        wd = 0 if w.dtype == torch.float32 else dt
        pd = 0 if _param_dtype(bn) in (None, torch.float32) else dt
        return _forward(ctx, _H16, (dt, wd, pd), x, w, gamma, beta, bn, relu, keep_z)

    backward = staticmethod(_backward)


def _fp32_here(t, x):
    return t is None or (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == x.device and t.is_contiguous())


def _plain_triple(linear, bn, relu_module, x, row_dtypes):
    """What `fusable` and `fusable16` ask alike: the three modules are the plain ones (no bias, subclass, hook or replaced forward), x is
    contiguous [n, cin] rows of one of `row_dtypes` on the GPU within the kernels' limits, and the BatchNorm's tensors come in pairs."""
    if not _ENABLED or type(linear) is not nn.Linear or linear.bias is not None or not _plain_forward(linear):
        return False
    if type(bn) is not nn.BatchNorm1d or not _plain_forward(bn) or bn.num_features != linear.out_features:
        return False
    if relu_module is not None and (type(relu_module) is not nn.ReLU or not _plain_forward(relu_module)):
        return False
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype in row_dtypes and x.dim() == 2 and x.is_contiguous()):
        return False
    n, cin = x.shape
    if cin != linear.in_features or not 1 <= cin <= MAX_IN or not 1 <= linear.out_features <= MAX_OUT:
        return False
    if n < (2 if bn.training else 1):   # torch raises for a single row in training mode: let it
        return False
    if (bn.weight is None) != (bn.bias is None) or (bn.running_mean is None) != (bn.running_var is None):
        return False
    t = bn.num_batches_tracked
    return t is None or (t.dtype == torch.int64 and t.device == x.device)


def fusable(linear, bn, relu_module, x):
    """The plain case of the (Linear, BatchNorm1d[, ReLU]) triple on rows x [n, cin] the fused op covers: fp32 everywhere, no autocast."""
    if not _plain_triple(linear, bn, relu_module, x, (torch.float32,)) or torch.is_autocast_enabled():
        return False
    return all(_fp32_here(t, x) for t in (linear.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var))


def linear_bn_relu(linear, bn, x, relu_module=None):
    """y = relu?(bn(linear(x))) for contiguous fp32 rows x [n, cin] on the GPU, or None when the fused path does not apply."""
    if not fusable(linear, bn, relu_module, x):
        return None
    keep_z = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, linear.weight, bn.weight, bn.bias))
    return _LinearBatchNormReLU.apply(x, linear.weight, bn.weight, bn.bias, bn, relu_module is not None, keep_z)


def fusable16(linear, bn, relu_module, x):
    """The plain case of the (Linear, BatchNorm1d[, ReLU]) triple on float16 / bfloat16 rows x [n, cin] the 16-bit op covers: the
    module, hook and forward checks of `fusable`, the dtype rules of `norm.fusable16`."""
    if not _plain_triple(linear, bn, relu_module, x, _DT16):
        return False
    autocast = torch.is_autocast_enabled()
    if autocast and not _ops.mixed_precision():   # (mixed precision: 16-bit rows under autocast are this route's case)
        return False
    w = linear.weight
    if not (torch.is_tensor(w) and w.device == x.device and w.is_contiguous()):
        return False
    if not (w.dtype == x.dtype or (w.dtype == torch.float32 and autocast)):   # an fp32 master weight: only where autocast would cast it
        return False
    pdt = _param_dtype(bn)
    if pdt is False or pdt not in (None, torch.float32, x.dtype):
        return False
    return all(t is None or (t.device == x.device and t.is_contiguous()) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))


def linear_bn_relu16(linear, bn, x, relu_module=None):
    """y = relu?(bn(linear(x))) for contiguous float16 / bfloat16 rows x [n, cin] on the GPU, or None when the 16-bit op does not apply."""
    if not fusable16(linear, bn, relu_module, x):
        return None
    keep_z = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, linear.weight, bn.weight, bn.bias))
    return _LinearBatchNormReLU16.apply(x, linear.weight, bn.weight, bn.bias, bn, relu_module is not None, keep_z)


def _is16(x):
    return torch.is_tensor(x) and x.dtype in _DT16


def try_rows(linear, bn, relu_module, x):
    """The triple on the rows x as one call where an op accepts it and pays at its shape - fp32 rows: `fusable` and `pays`; float16 /
    bfloat16 rows: `fusable16` and `pays16` - or None.  What `run_rows`, fv2p_model.run_rows and BEVGridPooling ask."""
    if _is16(x):
        if fusable16(linear, bn, relu_module, x) and pays16(x.shape[0], linear.in_features, linear.out_features, x.dtype):
            return linear_bn_relu16(linear, bn, x, relu_module)
        return None
    if fusable(linear, bn, relu_module, x) and pays(x.shape[0], linear.in_features, linear.out_features):
        return linear_bn_relu(linear, bn, x, relu_module)
    return None


def run_rows(mods, x):
    """The modules `mods` (a Sequential of Linear / BatchNorm1d / ReLU / ...) applied to the rows x in order, with every
    (Linear, BatchNorm1d[, ReLU]) run that `fusable` (fp32 rows) or `fusable16` (16-bit rows) accepts and that pays at its shape
    (`pays` / `pays16`) as one call.  Every other module runs as itself."""
    mods = list(mods)
    i = 0
    while i < len(mods):
        m = mods[i]
        if type(m) is nn.Linear and i + 1 < len(mods) and type(mods[i + 1]) is nn.BatchNorm1d:
            bn = mods[i + 1]
            relu = mods[i + 2] if i + 2 < len(mods) and type(mods[i + 2]) is nn.ReLU else None
            y = try_rows(m, bn, relu, x)
            if y is None and relu is not None:
                y = try_rows(m, bn, None, x)   # the ReLU module is not a plain one: the pair alone, then the module
                if y is not None:
                    relu = None
            if y is not None:
                x = y
                i += 2 + (relu is not None)
                continue
        x = m(x)
        i += 1
    return x
