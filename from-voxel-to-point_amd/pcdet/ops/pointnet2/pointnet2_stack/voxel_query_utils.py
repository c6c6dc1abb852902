"""VoxelQuery / VoxelQueryAndGrouping behind the names of the reference's
pcdet/ops/pointnet2/pointnet2_stack/voxel_query_utils.py:10-111 (Voxel R-CNN style neighbour-voxel grouping)."""
import torch
import torch.nn as nn

from ... import _glue as G
from . import pointnet2_utils


def _voxel_query(saved, max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices):
    """new_coords (M, 4) [b, z, y, x] voxel of every query, point_indices (B, Z, Y, X) voxel -> point row (or -1)
    -> (idx (M, nsample) GLOBAL point rows, empty_ball_mask (M)); empty queries come back as row 0."""
    m = new_coords.shape[0]
    _, z, y, x = point_indices.shape
    rz, ry, rx = max_range
    idx = torch.zeros((m, nsample), dtype=torch.int32, device=xyz.device)
    i32 = lambda t: t if t.dtype == torch.int32 else t.int()
    G.run("fv2p_voxel_query_stack", m, z, y, x, nsample, float(radius), rz, ry, rx, new_xyz, xyz, i32(new_coords), i32(point_indices), idx)
    empty = idx[:, 0] == -1
    idx[empty] = 0
    return idx, empty


VoxelQuery = G.autograd_op("VoxelQuery", _voxel_query)
voxel_query = VoxelQuery.apply


def local_rows(idx, empty, starts, batch_ids):
    """Global point rows (M, S) of the voxel query -> rows local to each query's own sample, as grouping_operation wants them:
    the start row of the query's sample is subtracted ONCE (starts (B) first row of every sample, batch_ids (M) sample of every
    query), empty queries come back as row 0.  Plain torch, on whatever device the tensors live."""
    idx = idx - starts.to(idx.device)[batch_ids.long()].view(-1, 1).to(idx.dtype)
    idx[empty] = 0
    return idx


class VoxelQueryAndGrouping(nn.Module):
    def __init__(self, max_range: int, radius: float, nsample: int):
        super().__init__()
        self.max_range, self.radius, self.nsample = max_range, radius, nsample

    def query(self, new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, voxel2point_indices):
        """-> (idx (M, S) GLOBAL point rows, empty_ball_mask (M)): the voxel query alone (empty queries hold row 0)."""
        if xyz.shape[0] != int(xyz_batch_cnt.sum()) or new_coords.shape[0] != int(new_xyz_batch_cnt.sum()):
            raise AssertionError("rows and batch counts disagree")
        return voxel_query(self.max_range, self.radius, self.nsample, xyz, new_xyz, new_coords, voxel2point_indices)

    def forward(self, new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, voxel2point_indices):
        """-> (grouped_features (M, C, S), grouped_xyz (M, 3, S), empty_ball_mask (M)).

        The query returns global rows; grouping wants rows local to the sample.  The reference's live conversion (:97-102) subtracts
        the start of the query's own sample, once, per batch-index mask; the per-block loop above it (:85-93) sits inside a string
        literal and never runs.  local_rows is that one conversion.  (Converting twice - what this class did before - is a no-op
        with one sample only: from the second sample on it gave global - 2 * start, rows of another sample or negative ones.)"""
        idx, empty = self.query(new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, voxel2point_indices)
        starts = torch.cumsum(xyz_batch_cnt, 0) - xyz_batch_cnt                                   # first row of every sample
        idx = local_rows(idx, empty, starts, new_coords[:, 0]).contiguous()
        grouped_xyz = pointnet2_utils.grouping_operation(xyz, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        grouped_features = pointnet2_utils.grouping_operation(features, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        return grouped_features, grouped_xyz, empty
