"""`pointnet2_batch_cuda` — the nine wrappers the reference binds (pointnet2_batch/src/pointnet2_api.cpp:10-24),
same positional arguments (ints first, then caller-allocated tensors)."""
import torch

import fv2p_native as _nat


def _go(name, dev_tensor, *args):
    _nat.require_cuda(*[a for a in args if isinstance(a, torch.Tensor)])
    for a in args:
        if isinstance(a, torch.Tensor) and not a.is_contiguous():
            raise _nat.Fv2pError(f"{name}: tensors must be contiguous")
    with _nat.device_guard(dev_tensor.device):
        _nat.call(name, *args, _nat.stream())
    return 1


def _det(name, grad_points_tensor, ws_args, *args):
    """Deterministic mode: `name`_gather writes the gradient into a fresh tensor, which is added to the caller's buffer once (the
    reference's contract: the buffer is accumulated into)."""
    g = torch.empty_like(grad_points_tensor)
    with _nat.device_guard(grad_points_tensor.device):
        ws = _nat.workspace(getattr(_nat.lib(), name + "_ws_bytes")(*ws_args), grad_points_tensor.device)
    _go(name + "_gather", grad_points_tensor, *args, g, ws, ws.numel())
    grad_points_tensor.add_(g)
    return 1


_DT16 = {torch.float16: 1, torch.bfloat16: 2}   # FV2P_DT_F16 / FV2P_DT_BF16 of include/fv2p_ops.h


def _dt16(name, src_tensor, dst_tensor):
    """-> the dtype code of the *_h entry point when the caller's feature tensors are float16 / bfloat16, None for the fp32 one.  The
    library reads both through pointers of one type: tensors that disagree, or a device tensor of another dtype, are an error."""
    if src_tensor.dtype != dst_tensor.dtype:
        raise TypeError(f"{name}: the tensors must have one dtype, got {src_tensor.dtype} and {dst_tensor.dtype}")
    if src_tensor.dtype in _DT16:
        return _DT16[src_tensor.dtype]
    if src_tensor.is_cuda and src_tensor.dtype != torch.float32:
        raise TypeError(f"{name}: float32, float16 and bfloat16 rows only, got {src_tensor.dtype}")
    return None


def _det_h(name, grad_points_tensor, dt, ws_args, *args):
    """16-bit gradients exist in the fixed-order form only: `name` writes into a fresh tensor, which is added to the caller's buffer
    once, as _det does."""
    g = torch.empty_like(grad_points_tensor)
    with _nat.device_guard(grad_points_tensor.device):
        ws = _nat.workspace(getattr(_nat.lib(), name + "_ws_bytes")(*ws_args), grad_points_tensor.device)
    _go(name, grad_points_tensor, *args, g, dt, ws, ws.numel())
    grad_points_tensor.add_(g)
    return 1


def ball_query_wrapper(b, n, m, radius, nsample, new_xyz_tensor, xyz_tensor, idx_tensor):
    return _go("fv2p_ball_query_batch", idx_tensor, b, n, m, float(radius), nsample, new_xyz_tensor, xyz_tensor, idx_tensor)


def group_points_wrapper(b, c, n, npoints, nsample, points_tensor, idx_tensor, out_tensor):
    dt = _dt16("group_points_wrapper", points_tensor, out_tensor)
    if dt is not None:
        return _go("fv2p_group_points_batch_h", out_tensor, b, c, n, npoints, nsample, points_tensor, idx_tensor, out_tensor, dt)
    return _go("fv2p_group_points_batch", out_tensor, b, c, n, npoints, nsample, points_tensor, idx_tensor, out_tensor)


def group_points_grad_wrapper(b, c, n, npoints, nsample, grad_out_tensor, idx_tensor, grad_points_tensor):
    dt = _dt16("group_points_grad_wrapper", grad_out_tensor, grad_points_tensor)
    if dt is not None:
        return _det_h("fv2p_group_points_batch_grad_h", grad_points_tensor, dt, (b, c, n, npoints, nsample), b, c, n, npoints, nsample,
                      grad_out_tensor, idx_tensor)
    if _nat.deterministic():
        return _det("fv2p_group_points_batch_grad", grad_points_tensor, (b, c, n, npoints, nsample), b, c, n, npoints, nsample,
                    grad_out_tensor, idx_tensor)
    return _go("fv2p_group_points_batch_grad", grad_out_tensor, b, c, n, npoints, nsample, grad_out_tensor, idx_tensor, grad_points_tensor)


def gather_points_wrapper(b, c, n, npoints, points_tensor, idx_tensor, out_tensor):
    dt = _dt16("gather_points_wrapper", points_tensor, out_tensor)
    if dt is not None:
        return _go("fv2p_gather_points_h", out_tensor, b, c, n, npoints, points_tensor, idx_tensor, out_tensor, dt)
    return _go("fv2p_gather_points", out_tensor, b, c, n, npoints, points_tensor, idx_tensor, out_tensor)


def gather_points_grad_wrapper(b, c, n, npoints, grad_out_tensor, idx_tensor, grad_points_tensor):
    dt = _dt16("gather_points_grad_wrapper", grad_out_tensor, grad_points_tensor)
    if dt is not None:
        return _det_h("fv2p_gather_points_grad_h", grad_points_tensor, dt, (b, c, n, npoints), b, c, n, npoints, grad_out_tensor, idx_tensor)
    if _nat.deterministic():
        return _det("fv2p_gather_points_grad", grad_points_tensor, (b, c, n, npoints), b, c, n, npoints, grad_out_tensor, idx_tensor)
    return _go("fv2p_gather_points_grad", grad_out_tensor, b, c, n, npoints, grad_out_tensor, idx_tensor, grad_points_tensor)


def furthest_point_sampling_wrapper(b, n, m, points_tensor, temp_tensor, idx_tensor):
    with _nat.device_guard(idx_tensor.device):   # scratch of the bucketed (lazy, bit-identical) kernel
        ws = _nat.workspace(_nat.lib().fv2p_furthest_point_sampling_ws_bytes(b, n), idx_tensor.device)
    return _go("fv2p_furthest_point_sampling", idx_tensor, b, n, m, points_tensor, temp_tensor, idx_tensor, ws, ws.numel())


def three_nn_wrapper(b, n, m, unknown_tensor, known_tensor, dist2_tensor, idx_tensor):
    return _go("fv2p_three_nn_batch", idx_tensor, b, n, m, unknown_tensor, known_tensor, dist2_tensor, idx_tensor)


def three_interpolate_wrapper(b, c, m, n, points_tensor, idx_tensor, weight_tensor, out_tensor):
    dt = _dt16("three_interpolate_wrapper", points_tensor, out_tensor)
    if dt is not None:
        return _go("fv2p_three_interpolate_batch_h", out_tensor, b, c, m, n, points_tensor, idx_tensor, weight_tensor, out_tensor, dt)
    return _go("fv2p_three_interpolate_batch", out_tensor, b, c, m, n, points_tensor, idx_tensor, weight_tensor, out_tensor)


def three_interpolate_grad_wrapper(b, c, n, m, grad_out_tensor, idx_tensor, weight_tensor, grad_points_tensor):
    dt = _dt16("three_interpolate_grad_wrapper", grad_out_tensor, grad_points_tensor)
    if dt is not None:
        return _det_h("fv2p_three_interpolate_batch_grad_h", grad_points_tensor, dt, (b, c, n, m), b, c, n, m, grad_out_tensor, idx_tensor,
                      weight_tensor)
    if _nat.deterministic():
        return _det("fv2p_three_interpolate_batch_grad", grad_points_tensor, (b, c, n, m), b, c, n, m, grad_out_tensor, idx_tensor,
                    weight_tensor)
    return _go("fv2p_three_interpolate_batch_grad", grad_out_tensor, b, c, n, m, grad_out_tensor, idx_tensor, weight_tensor, grad_points_tensor)
