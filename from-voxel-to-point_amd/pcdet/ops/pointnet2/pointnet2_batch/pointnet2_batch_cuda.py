"""`pointnet2_batch_cuda` — the nine wrappers the reference binds (pointnet2_batch/src/pointnet2_api.cpp:10-24),
same positional arguments (ints first, then caller-allocated tensors).  float16 / bfloat16 feature tensors reach the *_h entry points;
a gradient wrapper accumulates into the caller's buffer (G.grad_route)."""
from ... import _glue as G


def ball_query_wrapper(b, n, m, radius, nsample, new_xyz_tensor, xyz_tensor, idx_tensor):
    G.run("fv2p_ball_query_batch", b, n, m, float(radius), nsample, new_xyz_tensor, xyz_tensor, idx_tensor)
    return 1


def group_points_wrapper(b, c, n, npoints, nsample, points_tensor, idx_tensor, out_tensor):
    dt = G.pair_16bit("group_points_wrapper", points_tensor, out_tensor)
    if dt is not None:
        G.run("fv2p_group_points_batch_h", b, c, n, npoints, nsample, points_tensor, idx_tensor, out_tensor, dt)
    else:
        G.run("fv2p_group_points_batch", b, c, n, npoints, nsample, points_tensor, idx_tensor, out_tensor)
    return 1


def group_points_grad_wrapper(b, c, n, npoints, nsample, grad_out_tensor, idx_tensor, grad_points_tensor):
    G.pair_16bit("group_points_grad_wrapper", grad_out_tensor, grad_points_tensor)
    G.grad_route("fv2p_group_points_batch_grad", grad_out_tensor, None, (b, c, n, npoints, nsample), (grad_out_tensor, idx_tensor),
                 (b, c, n, npoints, nsample), into=grad_points_tensor)
    return 1


def gather_points_wrapper(b, c, n, npoints, points_tensor, idx_tensor, out_tensor):
    dt = G.pair_16bit("gather_points_wrapper", points_tensor, out_tensor)
    if dt is not None:
        G.run("fv2p_gather_points_h", b, c, n, npoints, points_tensor, idx_tensor, out_tensor, dt)
    else:
        G.run("fv2p_gather_points", b, c, n, npoints, points_tensor, idx_tensor, out_tensor)
    return 1


def gather_points_grad_wrapper(b, c, n, npoints, grad_out_tensor, idx_tensor, grad_points_tensor):
    G.pair_16bit("gather_points_grad_wrapper", grad_out_tensor, grad_points_tensor)
    G.grad_route("fv2p_gather_points_grad", grad_out_tensor, None, (b, c, n, npoints), (grad_out_tensor, idx_tensor), (b, c, n, npoints),
                 into=grad_points_tensor)
    return 1


def furthest_point_sampling_wrapper(b, n, m, points_tensor, temp_tensor, idx_tensor):
    ws = G.scratch("fv2p_furthest_point_sampling_ws_bytes", idx_tensor.device, b, n)   # scratch of the bucketed (lazy, bit-identical) kernel
    G.run("fv2p_furthest_point_sampling", b, n, m, points_tensor, temp_tensor, idx_tensor, ws, ws.numel())
    return 1


def three_nn_wrapper(b, n, m, unknown_tensor, known_tensor, dist2_tensor, idx_tensor):
    G.run("fv2p_three_nn_batch", b, n, m, unknown_tensor, known_tensor, dist2_tensor, idx_tensor)
    return 1


def three_interpolate_wrapper(b, c, m, n, points_tensor, idx_tensor, weight_tensor, out_tensor):
    dt = G.pair_16bit("three_interpolate_wrapper", points_tensor, out_tensor)
    if dt is not None:
        G.run("fv2p_three_interpolate_batch_h", b, c, m, n, points_tensor, idx_tensor, weight_tensor, out_tensor, dt)
    else:
        G.run("fv2p_three_interpolate_batch", b, c, m, n, points_tensor, idx_tensor, weight_tensor, out_tensor)
    return 1


def three_interpolate_grad_wrapper(b, c, n, m, grad_out_tensor, idx_tensor, weight_tensor, grad_points_tensor):
    G.pair_16bit("three_interpolate_grad_wrapper", grad_out_tensor, grad_points_tensor)
    G.grad_route("fv2p_three_interpolate_batch_grad", grad_out_tensor, None, (b, c, n, m), (grad_out_tensor, idx_tensor, weight_tensor),
                 (b, c, n, m), into=grad_points_tensor)
    return 1
