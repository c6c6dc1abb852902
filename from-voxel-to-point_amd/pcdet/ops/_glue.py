"""Shared plumbing of the Python ops layer: one helper that issues a C-ABI call of libfv2p_ops.so on the caller's stream, one
that turns a pair of plain functions into a torch.autograd.Function, and the policy of which entry point a call reaches given its
tensors' dtype and the deterministic switch (DT16, the dtype guards, grad_route).  The op modules next to this file describe each
operator as `forward(saved, *inputs)` / `backward(saved, *grads)` on top of these; nothing here falls back to the CPU."""
import torch
from torch.autograd import Function

import fv2p_native as _nat


def run(symbol, *args):
    """Validates the tensor arguments (device, contiguity) and calls `symbol` with the current stream appended."""
    tensors = [a for a in args if torch.is_tensor(a)]
    _nat.require_cuda(*tensors)
    for t in tensors:
        if not t.is_contiguous():
            raise _nat.Fv2pError(f"{symbol}: tensors must be contiguous")
    with _nat.device_guard(tensors[0].device):
        return _nat.call(symbol, *args, _nat.stream())


def scratch(nbytes_symbol, device, *size_args):
    """Workspace tensor of the size the library asks for (grow-only, per device and stream)."""
    with _nat.device_guard(device):
        return _nat.workspace(getattr(_nat.lib(), nbytes_symbol)(*size_args), device)


def new(like, shape, dtype=torch.float32, fill=None):
    t = torch.empty(shape, dtype=dtype, device=like.device)
    return t if fill is None else t.fill_(fill)


# 16-bit storage formats of the *_h entry points (FV2P_DT_F16 / FV2P_DT_BF16 of include/fv2p_ops.h)
DT16 = {torch.float16: 1, torch.bfloat16: 2}


def rows_16bit(op, t):
    """-> True for float16 / bfloat16 rows (the *_h entry points), False for the fp32 ones.  The library reads the rows through a
    pointer of that type and nothing is cast on the way, so a device tensor of any other dtype is an error.  (A host tensor never
    reaches the library: run refuses it; the CPU mirror of the tests, oracle/backend.py, answers the fp32 call names for float32 and
    float64 host tensors alike.)"""
    if t.dtype in DT16:
        return True
    if t.is_cuda and t.dtype != torch.float32:
        raise TypeError(f"{op}: float32, float16 and bfloat16 rows only, got {t.dtype}")
    return False


def pair_16bit(op, src, dst):
    """-> the dtype code of the *_h entry point when a caller-allocated source and destination are float16 / bfloat16, None for the
    fp32 one.  The library reads both through pointers of one type: tensors that disagree, or a device tensor of another dtype, are an
    error."""
    if src.dtype != dst.dtype:
        raise TypeError(f"{op}: the tensors must have one dtype, got {src.dtype} and {dst.dtype}")
    return DT16[src.dtype] if rows_16bit(op, src) else None


def one_dtype(op, nouns, *tensors, advice="nothing is cast here"):
    """The one dtype of a call's floating operands (None for an absent one): float32 (the fp32 kernels) or a key of DT16 (the 16-bit
    kernels).  Nothing is converted on the way, so every operand has to have it."""
    dts = {t.dtype for t in tensors if t is not None}
    if len(dts) > 1:
        raise TypeError(f"{op}: {nouns} must share one dtype, got " + ", ".join(sorted(str(d) for d in dts)) + f" ({advice})")
    dt = dts.pop()
    if dt != torch.float32 and dt not in DT16:
        raise NotImplementedError(f"{op}: float32, float16 and bfloat16 only, got {dt}")
    return dt


def grad_route(name, grad, shape, sizes, tensors, ws_sizes, *, atomic_sizes=None, gather=False, into=None, dtype=torch.float32):
    """The gradient of an op that sums into rows, by the one rule of its three entry points (`name` is the atomic one):
      float16 / bfloat16 `grad`      `name`_h: the fixed-order form is the only one (fp32 sums in the order of fv2p_scatter_add, one
                                     rounding), whatever the switches say; output of the gradient's dtype, workspace `name`_h_ws_bytes
      deterministic() or `gather`    `name`_gather: fixed order, no float atomics, no zero fill; workspace `name`_ws_bytes
      otherwise                      zero fill + `name` (float atomics)
    `sizes` / `tensors` are the call's leading integers and its input tensors, `ws_sizes` the workspace query's arguments,
    `atomic_sizes` the atomic form's integers where they differ, `dtype` the output's on the two fp32 routes.  `into` is the
    ext-module contract "the caller's buffer is accumulated into": the atomic form runs on the buffer itself, the fixed-order forms
    write a fresh tensor that is added to it once.  -> the gradient (`into` when given)."""
    dt = DT16.get(grad.dtype)
    if dt is None and not gather and not _nat.deterministic():
        g = torch.zeros(shape, dtype=dtype, device=grad.device) if into is None else into
        run(name, *(sizes if atomic_sizes is None else atomic_sizes), *tensors, g)
        return g
    g = torch.empty(shape, dtype=grad.dtype if dt else dtype, device=grad.device) if into is None else torch.empty_like(into)
    if dt:
        ws = scratch(name + "_h_ws_bytes", grad.device, *ws_sizes)
        run(name + "_h", *sizes, *tensors, g, dt, ws, ws.numel())
    else:
        ws = scratch(name + "_ws_bytes", grad.device, *ws_sizes)
        run(name + "_gather", *sizes, *tensors, g, ws, ws.numel())
    return g if into is None else into.add_(g)


def autograd_op(name, forward, backward=None, doc=None):
    """class `name`(Function) with forward(ctx, *inputs) = forward(ctx.saved, *inputs) and, when `backward` is given,
    backward(ctx, *grads) = backward(ctx.saved, *grads); without it every input gets a None gradient (index-valued ops)."""

    def _forward(ctx, *inputs):
        ctx.saved = {}
        ctx.n_inputs = len(inputs)
        return forward(ctx.saved, *inputs)

    def _backward(ctx, *grads):
        if backward is None:
            return (None,) * ctx.n_inputs
        out = backward(ctx.saved, *grads)
        out = out if isinstance(out, tuple) else (out,)
        return out + (None,) * (ctx.n_inputs - len(out))

    return type(name, (Function,), {"forward": staticmethod(_forward), "backward": staticmethod(_backward), "__doc__": doc or forward.__doc__})
