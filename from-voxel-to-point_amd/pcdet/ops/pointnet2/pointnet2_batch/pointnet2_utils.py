"""Batched pointnet2 operators behind the names of the reference's
pcdet/ops/pointnet2/pointnet2_batch/pointnet2_utils.py:10-380 (FurthestPointSampling, GatherOperation, ThreeNN, ThreeInterpolate,
GroupingOperation, BallQuery and their `.apply` aliases, QueryAndGroup, GroupAll, top3_interpolate[_with_grad]).

Each operator is a forward / backward function pair calling the C ABI directly (pcdet/ops/_glue.py); the ext-module name
`pointnet2_batch_cuda` with the reference's wrapper signatures lives next to this file for third-party callers."""
import torch
import torch.nn as nn

from ... import _glue as G
from ..._glue import rows_16bit as _rows_16bit   # kept under its earlier name here beside _coords_f32
from ..pointnet2_stack import pointnet2_utils as _stack


def _coords_f32(op, *tensors):
    """Coordinates are float32 only: their kernels read them through a float pointer, and 16 bits cannot carry metres anyway.  As for
    the feature rows (_rows_16bit) only a device tensor is judged; host tensors belong to the CPU mirror of the tests."""
    for t in tensors:
        if t.is_cuda and t.dtype != torch.float32:
            raise TypeError(f"{op}: float32 coordinates only, got {t.dtype}")


def _one_dtype(op, saved, grad):
    """The gradient has a dtype the library serves, and it is the dtype of the forward's features."""
    h = _rows_16bit(op, grad)
    fwd = saved.get("dtype", grad.dtype)
    if fwd != grad.dtype and (h or fwd in G.DT16):   # host tensors of the CPU mirror (float64 features, float32 output) are not judged
        raise TypeError(f"{op}: features and gradient must have one dtype, got {fwd} and {grad.dtype}")


# ---- sampling / gathering ------------------------------------------------------------------------------------------------------
def _fps(saved, xyz, npoint):
    """xyz (B, N, 3) -> (B, npoint) int32: index 0 first, then the farthest remaining point each round."""
    _coords_f32("furthest_point_sample", xyz)
    b, n, _ = xyz.shape
    idx = G.new(xyz, (b, npoint), torch.int32)
    running = G.new(xyz, (b, n), fill=1e10)
    ws = G.scratch("fv2p_furthest_point_sampling_ws_bytes", xyz.device, b, n)
    G.run("fv2p_furthest_point_sampling", b, n, npoint, xyz, running, idx, ws, ws.numel())
    return idx


def _gather(saved, features, idx):
    """features (B, C, N), idx (B, M) -> (B, C, M)."""
    h = _rows_16bit("gather_operation", features)
    b, c, n = features.shape
    m = idx.shape[1]
    out = G.new(features, (b, c, m), features.dtype if h else torch.float32)
    if not h:
        G.run("fv2p_gather_points", b, c, n, m, features, idx, out)
    else:   # 16-bit elements are copied as they are
        G.run("fv2p_gather_points_h", b, c, n, m, features, idx, out, G.DT16[features.dtype])
    saved.update(idx=idx, shape=(b, c, n, m), dtype=features.dtype)
    return out


def _gather_grad(saved, grad):
    b, c, n, m = saved["shape"]
    _one_dtype("gather_operation gradient", saved, grad)
    return G.grad_route("fv2p_gather_points_grad", grad, (b, c, n), (b, c, n, m), (grad.contiguous(), saved["idx"]), (b, c, n, m))


# ---- nearest neighbours and interpolation -------------------------------------------------------------------------------------------
def _three_nn(saved, unknown, known):
    """unknown (B, N, 3), known (B, M, 3) -> (distances (B, N, 3), indices (B, N, 3)) of the three nearest known points."""
    _coords_f32("three_nn", unknown, known)
    b, n, _ = unknown.shape
    d2 = G.new(unknown, (b, n, 3))
    idx = G.new(unknown, (b, n, 3), torch.int32)
    G.run("fv2p_three_nn_batch", b, n, known.shape[1], unknown, known, d2, idx)
    return d2.sqrt(), idx


def _interp(saved, features, idx, weight):
    """features (B, C, M), idx / weight (B, N, 3) -> (B, C, N)."""
    h = _rows_16bit("three_interpolate", features)
    b, c, m = features.shape
    n = idx.shape[1]
    out = G.new(features, (b, c, n), features.dtype if h else torch.float32)
    if not h:
        G.run("fv2p_three_interpolate_batch", b, c, m, n, features, idx, weight, out)
    else:   # fp32 arithmetic on the widened values, one rounding; the weight stays float32
        weight = weight.float() if weight.dtype in G.DT16 else weight
        G.run("fv2p_three_interpolate_batch_h", b, c, m, n, features, idx, weight, out, G.DT16[features.dtype])
    saved.update(idx=idx, weight=weight, shape=(b, c, m, n), dtype=features.dtype)
    return out


def _interp_grad(saved, grad):
    b, c, m, n = saved["shape"]
    _one_dtype("three_interpolate gradient", saved, grad)
    return G.grad_route("fv2p_three_interpolate_batch_grad", grad, (b, c, m), (b, c, n, m),
                        (grad.contiguous(), saved["idx"], saved["weight"]), (b, c, n, m))


# ---- ball query and grouping ----------------------------------------------------------------------------------------------------------
def _ball(saved, radius, nsample, xyz, new_xyz):
    """xyz (B, N, 3), new_xyz (B, M, 3) -> (B, M, nsample) int32, the first nsample points within `radius` in index order."""
    _coords_f32("ball_query", xyz, new_xyz)
    b, n, _ = xyz.shape
    m = new_xyz.shape[1]
    idx = torch.zeros((b, m, nsample), dtype=torch.int32, device=xyz.device)
    G.run("fv2p_ball_query_batch", b, n, m, float(radius), nsample, new_xyz, xyz, idx)
    return idx


def _group(saved, features, idx):
    """features (B, C, N), idx (B, M, S) -> (B, C, M, S)."""
    h = _rows_16bit("grouping_operation", features)
    b, c, n = features.shape
    _, m, s = idx.shape
    out = G.new(features, (b, c, m, s), features.dtype if h else torch.float32)
    if not h:
        G.run("fv2p_group_points_batch", b, c, n, m, s, features, idx, out)
    else:   # 16-bit elements are copied as they are
        G.run("fv2p_group_points_batch_h", b, c, n, m, s, features, idx, out, G.DT16[features.dtype])
    saved.update(idx=idx, shape=(b, c, n, m, s), dtype=features.dtype)
    return out


def _group_grad(saved, grad):
    b, c, n, m, s = saved["shape"]
    _one_dtype("grouping_operation gradient", saved, grad)
    return G.grad_route("fv2p_group_points_batch_grad", grad, (b, c, n), (b, c, n, m, s), (grad.contiguous(), saved["idx"]), (b, c, n, m, s))


FurthestPointSampling = G.autograd_op("FurthestPointSampling", _fps)
GatherOperation = G.autograd_op("GatherOperation", _gather, _gather_grad)
ThreeNN = G.autograd_op("ThreeNN", _three_nn)
ThreeInterpolate = G.autograd_op("ThreeInterpolate", _interp, _interp_grad)
GroupingOperation = G.autograd_op("GroupingOperation", _group, _group_grad)
BallQuery = G.autograd_op("BallQuery", _ball)
furthest_point_sample, gather_operation = FurthestPointSampling.apply, GatherOperation.apply
three_nn, three_interpolate = ThreeNN.apply, ThreeInterpolate.apply
grouping_operation, ball_query = GroupingOperation.apply, BallQuery.apply


class QueryAndGroup(nn.Module):
    """Ball query around new_xyz, then the neighbours' centred coordinates (and features) gathered into (B, 3 + C, M, S)."""

    def __init__(self, radius: float, nsample: int, use_xyz: bool = True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, new_xyz, features=None):
        idx = ball_query(self.radius, self.nsample, xyz, new_xyz)
        rel = grouping_operation(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)
        if features is None:
            assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
            return rel
        grouped = grouping_operation(features, idx)
        if self.use_xyz and grouped.dtype in G.DT16:
            rel = rel.to(grouped.dtype)   # 16-bit features stay 16-bit (cat would promote them); the offsets are bounded by the radius
        return torch.cat([rel, grouped], dim=1) if self.use_xyz else grouped


class GroupAll(nn.Module):
    """One group holding every point: (B, 3 + C, 1, N).  With 16-bit features and use_xyz the result keeps torch's promotion to the
    coordinates' float32: these are absolute coordinates in metres, which 16 bits cannot carry (QueryAndGroup's are offsets inside
    the ball and are cast)."""

    def __init__(self, use_xyz: bool = True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        coords = xyz.transpose(1, 2).unsqueeze(2)
        if features is None:
            return coords
        return torch.cat([coords, features.unsqueeze(2)], dim=1) if self.use_xyz else features.unsqueeze(2)


def _inverse_distance_weights(dist):
    w = 1.0 / (dist + 1e-8)
    return w / w.sum(dim=-1, keepdim=True)


def top3_interpolate(xyz, new_xyz, feats, nsamples=None):
    """Features feats (N, C) at xyz (N, 3) interpolated onto new_xyz (M, 3) from the three nearest sources with
    inverse-distance weights -> (M, C); the gradient reaches feats only (Voxel-to-Point decoder, reference :292-326).  float16 /
    bfloat16 feats give a result and a gradient of their dtype (the stacked three_interpolate on the rows as they are)."""
    if not (xyz.dim() == new_xyz.dim() == feats.dim() == 2):
        raise NotImplementedError
    dist, idx = three_nn(new_xyz.unsqueeze(0).contiguous(), xyz.unsqueeze(0).contiguous())
    if feats.dtype in G.DT16:   # (N, C) rows are the stacked op's layout already: no transposes, forward or backward
        return _stack.three_interpolate(feats.contiguous(), idx[0], _inverse_distance_weights(dist)[0])
    out = three_interpolate(feats.t().unsqueeze(0).contiguous(), idx, _inverse_distance_weights(dist))
    return out[0].t()


def top3_interpolate_with_grad(xyz, new_xyz, feats, nsamples=None):
    """Same interpolation with the weights recomputed from gathered coordinates, so that gradients also reach xyz and
    new_xyz (reference :329-380)."""
    if not (xyz.dim() == new_xyz.dim() == feats.dim() == 2):
        raise NotImplementedError
    _, idx = three_nn(new_xyz.detach().unsqueeze(0).contiguous(), xyz.unsqueeze(0).contiguous())
    near_xyz = grouping_operation(xyz.t().unsqueeze(0).contiguous(), idx)[0].permute(1, 2, 0)        # (M, 3, 3)
    near_feats = grouping_operation(feats.t().unsqueeze(0).contiguous(), idx)[0].permute(1, 2, 0)    # (M, 3, C)
    weight = _inverse_distance_weights((near_xyz - new_xyz.unsqueeze(1)).norm(dim=-1))
    if feats.dtype in G.DT16:   # grouped in 16 bits, the weighted sum in fp32, one rounding
        return (near_feats.float() * weight.unsqueeze(-1)).sum(dim=1).to(feats.dtype)
    return (near_feats * weight.unsqueeze(-1)).sum(dim=1)
