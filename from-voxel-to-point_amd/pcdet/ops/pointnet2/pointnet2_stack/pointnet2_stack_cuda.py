"""`pointnet2_stack_cuda` — the eight wrappers the reference binds (pointnet2_stack/src/pointnet2_api.cpp:11-23),
same positional arguments; outputs are caller-allocated and filled in place.  float16 / bfloat16 feature tensors reach the *_h entry
points; a gradient wrapper accumulates into the caller's buffer (G.grad_route)."""
import torch

from ... import _glue as G


def _i32(t):
    return t if t.dtype == torch.int32 else t.int()


def ball_query_wrapper(B, M, radius, nsample, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, idx):
    G.run("fv2p_ball_query_stack", B, M, float(radius), nsample, new_xyz, _i32(new_xyz_batch_cnt), xyz, _i32(xyz_batch_cnt), idx)
    return 1


def voxel_query_wrapper(M, R1, R2, R3, nsample, radius, z_range, y_range, x_range, new_xyz, xyz, new_coords, point_indices, idx):
    G.run("fv2p_voxel_query_stack", M, R1, R2, R3, nsample, float(radius), z_range, y_range, x_range, new_xyz, xyz, _i32(new_coords),
          _i32(point_indices), idx)
    return 1


def furthest_point_sampling_wrapper(b, n, m, points_tensor, temp_tensor, idx_tensor):
    ws = G.scratch("fv2p_furthest_point_sampling_ws_bytes", idx_tensor.device, b, n)   # scratch of the bucketed (lazy, bit-identical) kernel
    G.run("fv2p_furthest_point_sampling", b, n, m, points_tensor, temp_tensor, idx_tensor, ws, ws.numel())
    return 1


def group_points_wrapper(B, M, C, nsample, features, features_batch_cnt, idx, idx_batch_cnt, out):
    dt = G.pair_16bit("group_points_wrapper", features, out)
    if dt is not None:
        G.run("fv2p_group_points_stack_h", B, M, C, features.shape[0], nsample, features, _i32(features_batch_cnt), idx, _i32(idx_batch_cnt),
              out, dt)
    else:
        G.run("fv2p_group_points_stack", B, M, C, nsample, features, _i32(features_batch_cnt), idx, _i32(idx_batch_cnt), out)
    return 1


def group_points_grad_wrapper(B, M, C, N, nsample, grad_out, idx, idx_batch_cnt, features_batch_cnt, grad_features):
    G.pair_16bit("group_points_grad_wrapper", grad_out, grad_features)
    G.grad_route("fv2p_group_points_stack_grad", grad_out, None, (B, M, C, N, nsample),
                 (grad_out, idx, _i32(idx_batch_cnt), _i32(features_batch_cnt)), (M, C, nsample), into=grad_features)
    return 1


def three_nn_wrapper(unknown, unknown_batch_cnt, known, known_batch_cnt, dist2, idx):
    G.run("fv2p_three_nn_stack", unknown_batch_cnt.shape[0], unknown.shape[0], known.shape[0], unknown, _i32(unknown_batch_cnt), known,
          _i32(known_batch_cnt), dist2, idx)
    return 1


def three_interpolate_wrapper(features, idx, weight, out):
    dt = G.pair_16bit("three_interpolate_wrapper", features, out)
    if dt is not None:
        G.run("fv2p_three_interpolate_stack_h", idx.shape[0], features.shape[1], features.shape[0], features, idx, weight, out, dt)
    else:
        G.run("fv2p_three_interpolate_stack", idx.shape[0], features.shape[1], features, idx, weight, out)
    return 1


def three_interpolate_grad_wrapper(grad_out, idx, weight, grad_features):
    G.pair_16bit("three_interpolate_grad_wrapper", grad_out, grad_features)
    n, c, m = idx.shape[0], grad_out.shape[1], grad_features.shape[0]
    G.grad_route("fv2p_three_interpolate_stack_grad", grad_out, None, (n, c, m), (grad_out, idx, weight), (n, c, m), atomic_sizes=(n, c),
                 into=grad_features)
    return 1
