"""Fused Voxel R-CNN RoI-grid pooling (csrc/voxel_pool.hip): what a grouper of NeighborVoxelSAModuleMSG does between mlps_in and
mlps_out with pool_method 'max_pool', without the grouped (M, C, S) and (M, 3, S) tensors:

    voxel_pool_max(F, xyz, new_xyz, idx, empty, conv, bn)[i, c] = max_s relu(F[idx[i, s], c] + bn(conv(xyz[idx[i, s]] - new_xyz[i]))[c])

F (N, C) the mlps_in rows, idx (M, S) int32 GLOBAL rows of the voxel query, empty (M) bool (an empty query pools relu(bn(0))),
conv the Conv2d(3, C, 1, bias=False) and bn the BatchNorm2d of mlps_pos.  The BatchNorm runs in the module's own mode: batch
statistics over the M * S positions (running statistics and num_batches_tracked move as torch moves them) or the running ones.
Gradients for F, conv.weight, bn.weight and bn.bias; one byte per (query, channel) is kept for them.  On the GPU only, for float32
rows outside autocast and for the float16 / bfloat16 rows that mlps_in hands over under a torch.autocast of that dtype (the *_h
entry points: out, grad_out and grad_F in the rows' dtype, coordinates, parameters and their gradients float32 as always):
`supported()` says whether the op takes a call, and the module runs its torch route when it does not."""
import torch
import torch.nn as nn

import fv2p_native as _nat

from ... import _glue as G


def _plain_forward(module):
    """No hooks, and `forward` is the class's own (the rule of spconv/norm.py, restated: this package does not import that one)."""
    return not (module._forward_hooks or module._forward_pre_hooks or module._backward_hooks) and "forward" not in module.__dict__


def _modules_ok(conv, bn):
    if type(conv) is not nn.Conv2d or type(bn) is not nn.BatchNorm2d or not _plain_forward(conv) or not _plain_forward(bn):
        return False
    if conv.in_channels != 3 or conv.kernel_size != (1, 1) or conv.stride != (1, 1) or conv.padding not in ((0, 0), "valid") or \
            conv.dilation != (1, 1) or conv.groups != 1 or conv.bias is not None or conv.padding_mode != "zeros":
        return False
    if not (bn.affine and bn.track_running_stats) or bn.weight is None or bn.bias is None or bn.running_mean is None or \
            bn.running_var is None or bn.num_batches_tracked is None or bn.num_features != conv.out_channels:
        return False
    return True


def supported(features, idx, conv, bn, xyz=None, new_xyz=None, m=None, s=None):
    """Whether voxel_pool_max takes this call.  idx may be None when the query has not run yet: then m and s give its shape."""
    if not (torch.is_tensor(features) and features.is_cuda and features.dim() == 2):
        return False
    # float32 rows outside autocast; 16-bit rows only under an autocast of their own dtype - the one situation in which the torch route
    # returns rows of that dtype too (outside autocast it promotes them to the float32 of the parameters)
    if torch.is_autocast_enabled():
        if features.dtype not in G.DT16 or torch.get_autocast_dtype("cuda") != features.dtype:
            return False
    elif features.dtype != torch.float32:
        return False
    if not _modules_ok(conv, bn):
        return False
    if idx is not None:
        if not (idx.is_cuda and idx.dtype == torch.int32 and idx.dim() == 2):
            return False
        m, s = idx.shape
    if m is None or s is None:
        return False
    for t in (xyz, new_xyz):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 3 and not t.requires_grad):
            return False
    if new_xyz is not None and new_xyz.shape[0] != m or xyz is not None and xyz.shape[0] != features.shape[0]:
        return False
    for t in (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var):
        if not (t.is_cuda and t.dtype == torch.float32 and t.device == features.device):
            return False
    if bn.num_batches_tracked.dtype != torch.int64 or bn.num_batches_tracked.device != features.device:
        return False
    n, c = features.shape
    if c != conv.out_channels or n < 1 or (bn.training and m * s < 2):
        return False
    lib = _nat.lib()
    ws_bytes = lib.fv2p_voxel_pool_backward_h_ws_bytes if features.dtype in G.DT16 else lib.fv2p_voxel_pool_backward_ws_bytes
    return bool(lib.fv2p_voxel_pool_supported(m, s, c)) and ws_bytes(m, s, c, n) > 0


def _fwd(saved, f, xyz, new_xyz, idx, empty, w, gamma, beta, bn, needs):
    n, c = f.shape
    m, s = idx.shape
    f, xyz, new_xyz, idx, w = f.contiguous(), xyz.contiguous(), new_xyz.contiguous(), idx.contiguous(), w.contiguous().view(c, 3)
    empty = empty.contiguous().view(torch.uint8) if empty.dtype == torch.bool else empty.contiguous()
    dt = G.DT16[f.dtype] if G.rows_16bit("voxel_pool_max", f) else None
    out = G.new(f, (m, c), f.dtype)
    arg = G.new(f, (m, c), torch.uint8) if any(needs) else None     # the winning sample: all that backward needs beside `keep`
    keep = G.new(f, (_nat.lib().fv2p_voxel_pool_saved_bytes(c) // 8,), torch.float64)
    ws = G.scratch("fv2p_voxel_pool_ws_bytes", f.device, m, s, c)
    training = bool(bn.training)
    momentum = -1.0 if bn.momentum is None else float(bn.momentum)
    G.run("fv2p_voxel_pool_forward_h" if dt else "fv2p_voxel_pool_forward", f, xyz, new_xyz, idx, empty, n, m, s, c, w, gamma, beta,
          bn.running_mean, bn.running_var, bn.num_batches_tracked, momentum, float(bn.eps), int(training), out, arg, keep, ws, ws.numel(),
          *((dt,) if dt else ()))
    saved.update(t=(xyz, new_xyz, idx, empty, w, gamma, out, arg, keep), dims=(n, m, s, c), training=training, needs=needs)
    return out


def _bwd(saved, grad):
    xyz, new_xyz, idx, empty, w, gamma, out, arg, keep = saved["t"]
    if arg is None:
        raise RuntimeError("voxel_pool_max: backward of a forward pass that ran without gradients enabled")
    n, m, s, c = saved["dims"]
    need_f, need_w, need_g, need_b = saved["needs"]
    dt = G.pair_16bit("voxel_pool_max: out and grad_out", out, grad)     # nothing is cast: grad_out has the rows' dtype
    g_f = G.new(grad, (n, c), out.dtype) if need_f else None
    g_w = G.new(grad, (c, 3)) if need_w else None
    g_g = G.new(grad, (c,)) if need_g else None
    g_b = G.new(grad, (c,)) if need_b else None
    ws = G.scratch("fv2p_voxel_pool_backward_h_ws_bytes" if dt else "fv2p_voxel_pool_backward_ws_bytes", grad.device, m, s, c, n)
    G.run("fv2p_voxel_pool_backward_h" if dt else "fv2p_voxel_pool_backward", xyz, new_xyz, idx, empty, n, m, s, c, w, gamma, out, arg, keep,
          grad.contiguous(), int(saved["training"]), g_f, g_w, g_g, g_b, ws, ws.numel(), *((dt,) if dt else ()))
    return g_f, None, None, None, None, (g_w.view(c, 3, 1, 1) if need_w else None), g_g, g_b


VoxelPoolMax = G.autograd_op("VoxelPoolMax", _fwd, _bwd, doc=__doc__)


def voxel_pool_max(features, xyz, new_xyz, idx, empty, conv, bn):
    """-> (M, C) pooled features, or None when `supported` declines (nothing has been touched then)."""
    if not supported(features, idx, conv, bn, xyz, new_xyz) or not (torch.is_tensor(empty) and empty.is_cuda and empty.shape == (idx.shape[0],)
                                                                    and empty.dtype in (torch.bool, torch.uint8)):
        return None
    grad_on = torch.is_grad_enabled()
    needs = tuple(bool(grad_on and t.requires_grad) for t in (features, conv.weight, bn.weight, bn.bias))
    return VoxelPoolMax.apply(features, xyz, new_xyz, idx, empty, conv.weight, bn.weight, bn.bias, bn, needs)
