"""Op-sequence replay of the FV2P detector's training step (BASELINE configs[2]: fv2p.yaml, car only).

The reference's Python never travels to the GPU box, so this harness re-declares the detector as a consumer of the
`pcdet.ops` boundary, module by module in the reference's topology (detector3d_template.py:21-24):

  MeanVFE -> VoxelResBackBone8x -> HeightCompression -> BaseBEVBackbone -> AnchorHeadSingle ->
  ResidualVoxelToPointDecoder -> PointHeadSimple -> IoUGuidedRoIHead -> three losses summed (detectors/fv2p.py:9-45)

with the layer shapes, thresholds and loss weights of tools/cfgs/kitti_models/FV2P/fv2p.yaml.  The hot-path work goes
through this repo's ops (spconv, pointnet2 stack/batch, iou3d_nms, roiaware/roipoint pools, BEV bilinear gather); the
dense 2-D convolutions and the small MLPs are plain torch modules, as in the reference.

Where the reference loops over the samples of a batch in Python with boolean-mask indexing and `.item()` round trips
(decoder :121-134, point targets point_head_template.py:79-120, anchor targets axis_aligned_target_assigner.py:45-130,
RoI sampling proposal_target_layer.py:92-143) the same arithmetic runs here on whole-batch tensors without host
synchronisation: every per-sample quantity is a fixed-shape tensor, padded ground-truth rows are all-zero
boxes that can match nothing.  Random sampling consumes uniforms drawn from one generator so that a CPU run of the same
code (tests: oracle-backed ops) sees the same draws.
"""
import math
import os
from functools import partial

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from pcdet.ops.iou3d_nms import iou3d_nms_cuda, iou3d_nms_utils
from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_modules as pn2_batch_modules
from pcdet.ops.pointnet2.pointnet2_batch import fused as pn2_fused
from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_utils as pn2_batch
from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as pn2_stack
from pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils
from pcdet.ops.roipoint_pool3d import roipoint_pool3d_utils
from pcdet.models.backbones_3d.pfe import bev_grid_pooling
from pcdet.ops.spconv import norm as _norm
from pcdet.ops.spconv import head as _head
from pcdet.ops.spconv import linear as _linear
from pcdet.ops.spconv import bev_entry as _bev_entry

import fv2p_native as _nat

from .backbone import VoxelResBackBone8x, bn_act

TWO_PI = 2.0 * math.pi


class FV2PConfig:
    """Numbers of fv2p.yaml + kitti_dataset.yaml that shape the step."""
    point_cloud_range = (0.0, -40.0, -3.0, 70.4, 40.0, 1.0)
    voxel_size = (0.05, 0.05, 0.1)
    grid_size = (1408, 1600, 40)
    max_points_per_voxel, max_voxels = 5, 16000
    num_point_features = 4
    # BaseBEVBackbone
    bev_layers, bev_strides, bev_filters = (5, 5), (1, 2), (128, 256)
    bev_up_strides, bev_up_filters = (1, 2), (256, 256)
    # AnchorHeadSingle (Car)
    # ANCHOR_GENERATOR_CONFIG of fv2p.yaml: three entries although CLASS_NAMES is ['Car'] — the reference's head has 6 anchors per
    # location, of which the Pedestrian / Cyclist ones never see a box of their class and are background throughout
    # (axis_aligned_target_assigner.py:57-83).  (size, bottom height, matched threshold, unmatched threshold) per entry; class ids 1..
    anchor_rotations = (0.0, 1.57)
    anchor_classes = (((3.9, 1.6, 1.56), -1.78, 0.6, 0.45), ((0.8, 0.6, 1.73), -0.6, 0.5, 0.35), ((1.76, 0.6, 1.73), -0.6, 0.5, 0.35))
    dir_offset, dir_limit_offset, num_dir_bins = 0.78539, 0.0, 2
    rpn_w = dict(cls=1.0, loc=2.0, dir=0.2)
    # decoder
    num_keypoints = 16384
    decode_levels = (("x_conv4", 8, 128, 256), ("x_conv3", 4, 64, 192), ("x_conv2", 2, 32, 160), ("x_conv1", 1, 16, 128))
    init_source, init_stride, init_channels = "x_conv4", 8, 128
    decoder_out = 128
    # PointHeadSimple
    point_cls_fc, gt_extra_width, point_cls_weight = (64, 64), (0.2, 0.2, 0.2), 4.0
    # IoUGuidedRoIHead
    nms_pre, nms_post, nms_thresh = 9000, 512, 0.8
    roi_per_image, fg_ratio = 128, 0.5
    cls_fg, cls_bg, cls_bg_lo, reg_fg, hard_bg_ratio = 0.75, 0.25, 0.1, 0.55, 0.8
    pool_extra_width, num_sampled_points, depth_normalizer = (3.2, 3.2, 3.2), 512, 70.0
    xyz_up, grid_size_roi = (128, 128), 6
    sa_radii, sa_nsamples, sa_mlps = (0.8, 1.6), (16, 32), ((64, 64), (64, 64))
    bev_pool_in, bev_pool_out = 512, 128
    interact_filters, cge_up, cge_interact, fuse_filters = (256, 256), (64, 64), (128,), (256,)
    cls_fc, reg_fc, dp_ratio = (256, 256), (256, 256), 0.3
    grad_norm_clip = 10.0
    key_stream = True              # key-point sampling on its own stream beside the two backbones (False: in line, where the decoder asks for it)
    point_branch_stream = True     # decoder + point head on their own stream (their backward then overlaps the dense convs')
    # instead: BEV backbone + anchor head + second-stage preparation on a side stream from the end of the sparse backbone on (34.3 vs
    # 38.4 ms per step).  Off by default: it hung the device queue in every run on two boxes of twelve; bench.py switches
    # it on under its supervisor, which falls back to this default when the measurement stalls
    dense_branch_stream = False


class FV2PWaymoConfig(FV2PConfig):
    """waymo_fv2p_e30.yaml + waymo_dataset.yaml (BASELINE configs[4]): one class (Vehicle), ~180 k points per cloud, 0.1 m voxels,
    five point features, three instead of five convs per BEV block; decoder, point head and RoI head as on KITTI."""
    point_cloud_range = (-75.2, -75.2, -2.0, 75.2, 75.2, 4.0)
    voxel_size = (0.1, 0.1, 0.15)
    grid_size = (1504, 1504, 40)
    max_voxels = 80000
    num_point_features = 5
    bev_layers = (3, 3)
    anchor_classes = (((4.7, 2.1, 1.7), 0.0, 0.55, 0.4),)     # waymo_fv2p_e30.yaml: Vehicle only


# ---------------------------------------------------------------- small shared pieces -----------------
# False: target assignment, target sampling and the first-stage losses run as their tensor formulations on the GPU too — what
# fv2p_harness.refstyle.reference_call_structure() switches to (the batch kernels of csrc/targets.hip have no counterpart in the
# reference, whose Python does this work op by op)
KERNEL_GLUE = True
LINEAR_CHUNK_ROWS = 1024   # run_rows: rows per chunk of a chunked Linear (see there)
FULL_NMS = False   # refstyle.py: nms_gpu without the NMS_CONFIG keywords = every survivor computed, as the reference's kernel does
_SIDE_STREAMS = {}
_CONSTS = {}
_CORNER_SIGNS = ((1, 1, -1), (1, -1, -1), (-1, -1, -1), (-1, 1, -1), (1, 1, 1), (1, -1, 1), (-1, -1, 1), (-1, 1, 1))


def dconst(like, values, dtype=torch.float32):
    """A small constant as a tensor on `like`'s device, uploaded once per (device, value): `like.new_tensor(list)` and indexing
    with a Python list both stage a pageable host buffer, and that copy makes the host wait for everything queued on the stream."""
    key = (like.device, dtype, values)
    t = _CONSTS.get(key)
    if t is None:
        t = _CONSTS[key] = torch.tensor(values, dtype=dtype, device=like.device)
    return t


def side_stream(role, device):
    """One HIP stream per (role, device) for the whole process.  Kept outside the modules: a stream is not copyable, and the
    CPU mirror of a model (oracle.spconv_cpu.cpu_mirror) is a deep copy of it.  The dense-branch stream is a high-priority
    stream: HIP takes its hardware queue from another pool than the four queues all default-priority streams of the process
    share (measured with the input-pipeline stream: a default-priority side stream waited 20 ms behind the training stream's
    queue, a high-priority one did not; the step time is the same, 33.5 - 34.0 ms).  FV2P_STREAM_PRIO overrides the set of
    high-priority roles (comma separated: dense, fps, point)."""
    key = (role, torch.device(device).index)
    if key not in _SIDE_STREAMS:
        high = role in os.environ.get("FV2P_STREAM_PRIO", "dense").split(",")
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device, priority=-1 if high else 0)
    return _SIDE_STREAMS[key]


def limit_period(val, offset, period):
    return val - torch.floor(val / period + offset) * period


def rotate_z(points, angle):
    """points (M, P, 3+), angle (M): rotation about z, x towards y for positive angles (common_utils.py:34-56)."""
    c, s = torch.cos(angle), torch.sin(angle)
    x, y = points[..., 0], points[..., 1]
    xr = x * c[:, None] - y * s[:, None]
    yr = x * s[:, None] + y * c[:, None]
    return torch.cat((xr.unsqueeze(-1), yr.unsqueeze(-1), points[..., 2:]), dim=-1)


def residual_encode(boxes, anchors):
    """ResidualCoder.encode_torch (box_coder_utils.py:13-46) on (..., 7) tensors."""
    a_sz = anchors[..., 3:6].clamp_min(1e-5)
    b_sz = boxes[..., 3:6].clamp_min(1e-5)
    diag = torch.sqrt(a_sz[..., 0:1] ** 2 + a_sz[..., 1:2] ** 2)
    xy = (boxes[..., 0:2] - anchors[..., 0:2]) / diag
    z = (boxes[..., 2:3] - anchors[..., 2:3]) / a_sz[..., 2:3]
    return torch.cat((xy, z, torch.log(b_sz / a_sz), boxes[..., 6:7] - anchors[..., 6:7]), dim=-1)


def residual_decode(enc, anchors):
    """ResidualCoder.decode_torch (box_coder_utils.py:48-81)."""
    a_sz = anchors[..., 3:6]
    diag = torch.sqrt(a_sz[..., 0:1] ** 2 + a_sz[..., 1:2] ** 2)
    xy = enc[..., 0:2] * diag + anchors[..., 0:2]
    z = enc[..., 2:3] * a_sz[..., 2:3] + anchors[..., 2:3]
    return torch.cat((xy, z, torch.exp(enc[..., 3:6]) * a_sz, enc[..., 6:7] + anchors[..., 6:7]), dim=-1)


def sigmoid_focal(logits, onehot, weights, alpha=0.25, gamma=2.0):
    """SigmoidFocalClassificationLoss.forward (loss_utils.py:52-82); weights broadcast over the class axis."""
    p = torch.sigmoid(logits)
    alpha_w = onehot * alpha + (1 - onehot) * (1 - alpha)
    pt = onehot * (1.0 - p) + (1.0 - onehot) * p
    bce = logits.clamp(min=0) - logits * onehot + torch.log1p(torch.exp(-logits.abs()))
    return alpha_w * pt.pow(gamma) * bce * weights.unsqueeze(-1)


def smooth_l1(diff, beta):
    n = diff.abs()
    return torch.where(n < beta, 0.5 * n * n / beta, n - 0.5 * beta)


def box_corners(boxes):
    """(M, 7) -> (M, 8, 3) corner order of box_utils.boxes_to_corners_3d (:28-53)."""
    t = dconst(boxes, _CORNER_SIGNS, boxes.dtype) / 2
    c = boxes[:, None, 3:6] * t[None]
    return rotate_z(c, boxes[:, 6]) + boxes[:, None, 0:3]


def corner_loss_lidar(pred, gt):
    """loss_utils.get_corner_loss_lidar (:217-241): per box the mean over the eight corners of smooth-L1(beta 1) of the corner
    distance to the ground-truth box or to its heading-flipped twin, whichever is nearer.  (N, 7) x (N, 7) -> (N,)."""
    pc, gc = box_corners(pred), box_corners(gt)
    gflip = box_corners(torch.cat((gt[:, :6], gt[:, 6:7] + math.pi), dim=1))
    dist = torch.minimum((pc - gc).norm(dim=2), (pc - gflip).norm(dim=2))
    return smooth_l1(dist, 1.0).mean(dim=1)


def nearest_bev_boxes(b):
    """boxes3d_lidar_to_aligned_bev_boxes (box_utils.py:337-348): (..., 7) -> (..., 4) axis-aligned footprint."""
    rot = limit_period(b[..., 6], 0.5, math.pi).abs()
    swap = (rot >= math.pi / 4).unsqueeze(-1)
    dims = torch.where(swap, b[..., 3:5].flip(-1), b[..., 3:5])
    return torch.cat((b[..., 0:2] - dims / 2, b[..., 0:2] + dims / 2), dim=-1)


def mlp1d(cin, widths, out=None, conv=False, bn_kw=None, dropout_after_first=None):
    """Linear/Conv1d + BatchNorm1d + ReLU stack, optionally closed by a biased projection."""
    mk = (lambda a, b, bias: nn.Conv1d(a, b, 1, bias=bias)) if conv else (lambda a, b, bias: nn.Linear(a, b, bias=bias))
    layers = []
    for i, w in enumerate(widths):
        layers += [mk(cin, w, False), nn.BatchNorm1d(w, **(bn_kw or {})), nn.ReLU()]
        if dropout_after_first is not None and i == 0:
            layers.append(nn.Dropout(dropout_after_first))
        cin = w
    if out is not None:
        layers.append(mk(cin, out, True))
    return nn.Sequential(*layers)


def run_rows(seq, x):
    """nn.Sequential of Linear / BatchNorm1d / ReLU over [N, C] rows, with every BatchNorm1d (+ReLU) pair as one fused op."""
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        if KERNEL_GLUE and type(m) is nn.Linear and i + 1 < len(mods) and type(mods[i + 1]) is nn.BatchNorm1d:
            # Linear -> BatchNorm1d [-> ReLU] as one op (csrc/linear_bn.hip) where it applies and measured faster at this shape
            relu = mods[i + 2] if i + 2 < len(mods) and type(mods[i + 2]) is nn.ReLU else None
            # (float16 / bfloat16 rows: the 16-bit formats of the same kernel source, by fusable16 and pays16)
            y = _linear.try_rows(m, mods[i + 1], relu, x)
            if y is not None:
                x = y
                i += 2 + (relu is not None)
                continue
        if isinstance(m, nn.BatchNorm1d) and x.dim() == 2:
            relu = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU) else None
            x = bn_act(m, x, relu)
            i += 1 + (relu is not None)
        elif (KERNEL_GLUE and type(m) is nn.Linear and x.dim() == 2 and x.is_cuda and x.shape[0] >= 4 * LINEAR_CHUNK_ROWS
              and x.shape[0] % LINEAR_CHUNK_ROWS == 0 and "forward" not in m.__dict__):
            # the same product in chunks of rows (rows_linear): autograd then forms the weight gradient as one batched product over the
            # chunks (K = 1024 each) and sums them, instead of ONE product with K = 49 152 rows and a 128 .. 256-wide output - eight to
            # sixteen output tiles on 256 CUs, 130 - 200 us each, 14 of them per step (profiles/r04_fv2p_kernel_stats.csv, `Cijk_Ailk_Bjlk`)
            x = rows_linear(x.reshape(-1, LINEAR_CHUNK_ROWS, x.shape[1]), m.weight, m.bias).reshape(x.shape[0], -1)
            i += 1
        else:
            x = m(x)
            i += 1
    return x


# ---------------------------------------------------------------- dense BEV part ----------------------
def run_maps(seq, x):
    """seq(x) for an nn.Sequential over dense maps, with every (BatchNorm2d, ReLU) pair as one fused op (pcdet.ops.spconv.norm:
    3 passes over the map forward and 5 backward instead of 5 and 8, the pre-activation never stored).  The module list is untouched."""
    return _norm.run_maps(seq, x) if KERNEL_GLUE else seq(x)


class BEVBackbone(nn.Module):
    """BaseBEVBackbone (base_bev_backbone.py:6-112) for LAYER_NUMS [5,5], strides [1,2], filters [128,256], up [1,2]->256."""

    def __init__(self, cfg, cin):
        super().__init__()
        bn = partial(nn.BatchNorm2d, eps=1e-3, momentum=0.01)
        self.blocks, self.deblocks = nn.ModuleList(), nn.ModuleList()
        for n, s, f, us, uf in zip(cfg.bev_layers, cfg.bev_strides, cfg.bev_filters, cfg.bev_up_strides, cfg.bev_up_filters):
            seq = [nn.ZeroPad2d(1), nn.Conv2d(cin, f, 3, stride=s, padding=0, bias=False), bn(f), nn.ReLU()]
            for _ in range(n):
                seq += [nn.Conv2d(f, f, 3, padding=1, bias=False), bn(f), nn.ReLU()]
            self.blocks.append(nn.Sequential(*seq))
            self.deblocks.append(nn.Sequential(nn.ConvTranspose2d(f, uf, us, stride=us, bias=False), bn(uf), nn.ReLU()))
            cin = f
        self.num_bev_features = sum(cfg.bev_up_filters)

    def forward(self, x):
        """x: the dense map [B, C * D, H, W], or the SparseConvTensor HeightCompression would make it from (height_compression.py:10-26)."""
        ups = []
        for blk, de in zip(self.blocks, self.deblocks):
            x = self._block(blk, x)
            ups.append(run_maps(de, x))   # (the 1 x 1 ConvTranspose2d of the first level issued as a 1 x 1 conv measured 0.15 ms per step slower)
        return torch.cat(ups, dim=1)

    @staticmethod
    def height_compression(sp):
        dense = sp.dense()
        return dense.view(dense.shape[0], dense.shape[1] * dense.shape[2], dense.shape[3], dense.shape[4])

    @staticmethod
    def _block(blk, x):
        """blk(x) with the leading ZeroPad2d(1) + Conv2d(padding=0) pair of the reference's block (base_bev_backbone.py:27-33) issued as
        one zero-padded convolution: the same sums, without the padded copy of the map (108 MB written and read again at the FV2P size,
        and its slice copy in the backward pass).  The module list keeps the reference's layout (state dicts load unchanged).
        A SparseConvTensor x (the first block) goes through that pair as a sparse convolution over its rows while its fill allows
        (pcdet.ops.spconv.bev_entry: no dense map, no products with its zeros), and through HeightCompression otherwise."""
        mods = list(blk)
        pair = (KERNEL_GLUE and len(mods) >= 2 and isinstance(mods[0], nn.ZeroPad2d) and type(mods[1]) is nn.Conv2d and "forward" not in mods[1].__dict__
                and tuple(mods[0].padding) == (1, 1, 1, 1) and tuple(mods[1].padding) == (0, 0) and mods[1].padding_mode == "zeros")
        if not torch.is_tensor(x):
            c = mods[1] if pair else None
            if (pair and c.bias is None and tuple(c.stride) == (1, 1) and tuple(c.dilation) == (1, 1) and c.groups == 1
                    and _bev_entry.route(x, c.weight) == "sparse"):
                return _norm.run_maps(mods[2:], _bev_entry.bev_entry_conv(x, c.weight))
            x = BEVBackbone.height_compression(x)
        if pair:
            c = mods[1]
            x = F.conv2d(x, c.weight, c.bias, c.stride, (1, 1), c.dilation, c.groups)
            mods = mods[2:]
        if KERNEL_GLUE:
            return _norm.run_maps(mods, x)
        for m in mods:
            x = m(x)
        return x


class AnchorLossFn(torch.autograd.Function):
    """fv2p_anchor_loss: focal + smooth-L1 (sin-difference heading) + direction-bin losses of AnchorHeadTemplate.get_loss
    (anchor_head_template.py:98-206) for a batch; the forward launch leaves the gradients with respect to the three logit tensors."""

    @staticmethod
    def forward(ctx, cls, box, dirs, labels, reg_t, anchor_rot, cfg):
        b, a = labels.shape
        out = cls.new_empty(4)
        dcls, dbox, ddirs = torch.empty_like(cls), torch.empty_like(box), torch.empty_like(dirs)
        with _nat.device_guard(cls.device):
            ws = _nat.workspace(int(_nat.lib().fv2p_anchor_loss_ws_bytes(b, a)), cls.device)
            _nat.call("fv2p_anchor_loss", cls, box, dirs, labels, reg_t, anchor_rot, b, a, 0.25, 1.0 / 9.0, float(cfg.dir_offset),
                      float(cfg.rpn_w["cls"]), float(cfg.rpn_w["loc"]), float(cfg.rpn_w["dir"]), out, dcls, dbox, ddirs, ws, ws.numel(), _nat.stream())
        ctx.save_for_backward(dcls, dbox, ddirs)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        dcls, dbox, ddirs = ctx.saved_tensors
        return dcls * g, dbox * g, ddirs * g, None, None, None, None


class RoiLossFn(torch.autograd.Function):
    """fv2p_roi_loss: the second-stage losses (IoUGuidedRoIHead.losses / reg_losses / corner_loss_lidar, with canonical_targets formed
    inside) of the sampled RoIs in one launch, which leaves the gradients with respect to the class logit and the [iou, 7 residuals] row."""

    @staticmethod
    def forward(ctx, rois, gt, iou, cls, reg8, cfg):
        r = cls.shape[0]
        rois, gt = rois.reshape(-1, 7).contiguous(), gt.reshape(-1, gt.shape[-1]).contiguous()
        iou, cls, reg8 = iou.reshape(-1).contiguous(), cls.contiguous(), reg8.contiguous()
        if not (rois.shape[0] == gt.shape[0] == iou.shape[0] == reg8.shape[0] == r and cls.numel() == r and reg8.shape[1] == 8):
            raise ValueError("RoiLossFn: rois (R, 7), gt (R, >= 7), iou (R), cls (R, 1) and reg (R, 8) must agree in R")
        out = cls.new_empty(5)
        dcls, dreg = torch.empty_like(cls), torch.empty_like(reg8)
        with _nat.device_guard(cls.device):
            _nat.call("fv2p_roi_loss", rois, gt, iou, cls, reg8, r, gt.shape[1], float(cfg.cls_fg), float(cfg.cls_bg),
                      cfg.cls_fg - cfg.cls_bg, float(cfg.reg_fg), (cfg.reg_fg - 0.5) * 2, 1.0 / 9.0, out, dcls, dreg, None, _nat.stream())
        ctx.save_for_backward(dcls, dreg)
        return out[0]   # out = {total, cls, reg, corner, iou}

    @staticmethod
    def backward(ctx, g):
        dcls, dreg = ctx.saved_tensors
        return None, None, None, dcls * g, dreg * g, None


class PointLossFn(torch.autograd.Function):
    """fv2p_point_loss: PointHead's focal loss over labels in {-1, 0, 1}, its logit gradient and the score sigmoid(logit) in one pass."""

    @staticmethod
    def forward(ctx, logits, labels, weight):
        logits, labels = logits.contiguous(), labels.contiguous()
        n = logits.numel()
        out = logits.new_empty(1)
        dlogits, score = torch.empty_like(logits), logits.new_empty(n)
        with _nat.device_guard(logits.device):
            ws = _nat.workspace(int(_nat.lib().fv2p_point_loss_ws_bytes(n)), logits.device)
            _nat.call("fv2p_point_loss", logits, labels, n, 0.25, float(weight), out, dlogits, score, ws, ws.numel(), _nat.stream())
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(score)
        return out[0], score

    @staticmethod
    def backward(ctx, g, _):
        dlogits, = ctx.saved_tensors
        return dlogits * g, None, None


def roi_grid_geometry(rois, g):
    """fv2p_roi_grid: what roi_streams reads of the RoI grids, from one launch.  rois (..., 7) float32 on the GPU, no gradient ->
    (local (R, g^3, 3) grid points in the roi's frame, x slowest; column (R, g^2, 3) world position of the lowest grid point of every
    (x, y) column; corners (R, 8, 3) half-extent corner offsets)."""
    if not (rois.is_cuda and rois.dtype == torch.float32) or rois.requires_grad:
        raise ValueError("roi_grid_geometry: float32 CUDA rois without gradient (IoUGuidedRoIHead.grid_points is the tensor form)")
    r = rois.reshape(-1, 7).contiguous()
    local, column, corners = r.new_empty(r.shape[0], g ** 3, 3), r.new_empty(r.shape[0], g * g, 3), r.new_empty(r.shape[0], 8, 3)
    with _nat.device_guard(r.device):
        _nat.call("fv2p_roi_grid", r, r.shape[0], g, local, column, corners, _nat.stream())
    return local, column, corners


def pool_points_in_frame(layer, depth_normalizer, key, feats, scores, rois):
    """fv2p_roipoint_pool3d_frame: RoIPointPool3d's selection on the enlarged boxes with the rows [x', y', z', score, depth, features]
    written in the roi's frame by the pool kernel itself.  key (B, N, 3), feats (B * N, C), scores (B * N), rois (B, M, 7) ->
    (B * M, S, 5 + C), no gradient (the reference pools under no_grad)."""
    with torch.no_grad():
        b, n, _ = key.shape
        m, c, s = rois.shape[1], feats.shape[1], layer.num_sampled_points
        rois = rois.contiguous()
        big, extra = rois.clone(), layer.pool_extra_width   # the boxes of the inside test: every side widened (a list) or scaled (a scalar)
        if isinstance(extra, (list, tuple)) and len(set(extra)) == 1:
            big[..., 3:6] += extra[0]   # a Python scalar becomes a kernel argument: no host-to-device copy
        elif isinstance(extra, (list, tuple)):
            for axis, e in enumerate(extra):
                big[..., 3 + axis] += e
        else:
            big[..., 3:6] += rois[..., 3:6] * extra
        pooled = feats.new_empty((b * m, s, 5 + c))
        empty = torch.empty((b, m), dtype=torch.int32, device=feats.device)
        with _nat.device_guard(feats.device):
            _nat.call("fv2p_roipoint_pool3d_frame", key.contiguous(), scores.detach().contiguous(), feats.detach().contiguous(), big, rois,
                      b, n, m, c, s, float(depth_normalizer), pooled, empty, _nat.stream())
    return pooled


class AnchorHead(nn.Module):
    """AnchorHeadSingle + AxisAlignedTargetAssigner for one class (anchor_head_single.py, anchor_head_template.py,
    axis_aligned_target_assigner.py:132-212), targets assigned for the whole batch at once."""

    def __init__(self, cfg, cin):
        super().__init__()
        self.cfg = cfg
        nr, nc = len(cfg.anchor_rotations), len(cfg.anchor_classes)
        na = nr * nc
        self.conv_cls = nn.Conv2d(cin, na, 1)
        self.conv_box = nn.Conv2d(cin, na * 7, 1)
        self.conv_dir_cls = nn.Conv2d(cin, na * cfg.num_dir_bins, 1)
        nn.init.constant_(self.conv_cls.bias, -math.log((1 - 0.01) / 0.01))
        nn.init.normal_(self.conv_box.weight, mean=0, std=0.001)
        # anchors [H, W, class, rot, 7] flattened (anchor_generator.py:20-61: align_center False -> linspace over the range; the
        # per-class sets concatenated the way AnchorHeadTemplate does it, torch.cat(self.anchors, dim=-3))
        r = cfg.point_cloud_range
        w, h = cfg.grid_size[0] // 8, cfg.grid_size[1] // 8
        xs = torch.arange(r[0], r[3] + 1e-5, step=(r[3] - r[0]) / (w - 1), dtype=torch.float32)
        ys = torch.arange(r[1], r[4] + 1e-5, step=(r[4] - r[1]) / (h - 1), dtype=torch.float32)
        a = torch.zeros(h, w, nc, nr, 7)
        a[..., 0] = xs.view(1, w, 1, 1)
        a[..., 1] = ys.view(h, 1, 1, 1)
        for c, (size, bottom, _, _) in enumerate(cfg.anchor_classes):
            a[:, :, c, :, 3:6] = torch.tensor(size)
            a[:, :, c, :, 2] = bottom
        a[..., 6] = torch.tensor(cfg.anchor_rotations).view(1, 1, 1, nr)
        a[..., 2] += a[..., 5] / 2                                              # bottom height -> box centre (anchor_generator.py:58)
        self.register_buffer("anchors", a.view(-1, 7), persistent=False)
        self.register_buffer("anchor_rot", a.view(-1, 7)[:, 6].contiguous(), persistent=False)
        for c in range(nc):   # the target assigner works class by class on that class's anchors (y, x, rot)
            ac = a[:, :, c].reshape(-1, 7).contiguous()
            self.register_buffer(f"anchors_c{c}", ac, persistent=False)
            self.register_buffer(f"anchor_bev_c{c}", nearest_bev_boxes(ac), persistent=False)

    @torch.no_grad()
    def assign(self, gt):
        """gt (B, G, 8) zero padded -> labels (B, A) in {-1, 0, cls}, reg targets (B, A, 7).  Class by class
        (AxisAlignedTargetAssigner.assign_targets :36-128): the anchors of entry c meet the boxes of class c + 1 only."""
        cfg = self.cfg
        nc, nr, b = len(cfg.anchor_classes), len(cfg.anchor_rotations), gt.shape[0]
        labels, regs = [], []
        for c, (_, _, matched, unmatched) in enumerate(cfg.anchor_classes):
            gt_c = gt if nc == 1 else torch.where((gt[..., 7:8] == c + 1), gt, torch.zeros_like(gt))   # other classes' rows become padding
            one = self.assign_one_kernel if (gt.is_cuda and gt.shape[-1] >= 8 and KERNEL_GLUE) else self.assign_one_tensor_ops
            lab, reg = one(gt_c, getattr(self, f"anchors_c{c}"), getattr(self, f"anchor_bev_c{c}"), matched, unmatched)
            labels.append(lab.view(b, -1, 1, nr))
            regs.append(reg.view(b, -1, 1, nr, 7))
        if nc == 1:
            return labels[0].view(b, -1), regs[0].view(b, -1, 7)
        return torch.cat(labels, dim=2).reshape(b, -1), torch.cat(regs, dim=2).reshape(b, -1, 7)

    def assign_tensor_ops(self, gt):
        """The same rule in torch ops only (the CPU path; the kernel is compared with it bit for bit)."""
        cfg = self.cfg
        nc, nr, b = len(cfg.anchor_classes), len(cfg.anchor_rotations), gt.shape[0]
        labels, regs = [], []
        for c, (_, _, matched, unmatched) in enumerate(cfg.anchor_classes):
            gt_c = gt if nc == 1 else torch.where((gt[..., 7:8] == c + 1), gt, torch.zeros_like(gt))
            lab, reg = self.assign_one_tensor_ops(gt_c, getattr(self, f"anchors_c{c}"), getattr(self, f"anchor_bev_c{c}"), matched, unmatched)
            labels.append(lab.view(b, -1, 1, nr))
            regs.append(reg.view(b, -1, 1, nr, 7))
        return torch.cat(labels, dim=2).reshape(b, -1), torch.cat(regs, dim=2).reshape(b, -1, 7)

    @staticmethod
    @torch.no_grad()
    def assign_one_kernel(gt, anchors, anchor_bev, matched, unmatched):
        # two launches for the batch (csrc/targets.hip); assign_one_tensor_ops is the same rule in torch ops
        b, g, a = gt.shape[0], gt.shape[1], anchors.shape[0]
        gt = gt.contiguous()
        gb = nearest_bev_boxes(gt[..., :7]).contiguous()
        labels = torch.empty((b, a), dtype=torch.int32, device=gt.device)
        reg = gt.new_empty(b, a, 7)
        with _nat.device_guard(gt.device):
            ws = _nat.workspace(int(_nat.lib().fv2p_anchor_assign_ws_bytes(b, g)), gt.device)
            _nat.call("fv2p_anchor_assign", anchor_bev, anchors, a, gb, gt, b, g, gt.shape[-1], float(matched), float(unmatched), labels, reg, ws,
                      ws.numel(), _nat.stream())
        return labels, reg

    @staticmethod
    @torch.no_grad()
    def assign_one_tensor_ops(gt, anchors, ab, matched, unmatched):
        gb = nearest_bev_boxes(gt[..., :7])                                     # (B, G, 4); ab (A, 4)
        lo = torch.maximum(ab[None, :, None, 0:2], gb[:, None, :, 0:2])
        hi = torch.minimum(ab[None, :, None, 2:4], gb[:, None, :, 2:4])
        inter = (hi - lo).clamp_min(0).prod(-1)                                 # (B, A, G)
        area_a = ((ab[:, 2] - ab[:, 0]) * (ab[:, 3] - ab[:, 1]))[None, :, None]
        area_g = ((gb[..., 2] - gb[..., 0]) * (gb[..., 3] - gb[..., 1]))[:, None, :]
        iou = inter / (area_a + area_g - inter).clamp_min(1e-6)
        a_max, a_arg = iou.max(dim=2)                                           # per anchor (first maximum, as numpy argmax)
        g_max = iou.max(dim=1).values                                           # per gt
        g_max = torch.where(g_max == 0, torch.full_like(g_max, -1.0), g_max)
        forced = (iou == g_max[:, None, :]).any(dim=2)
        cls = torch.gather(gt[..., 7], 1, a_arg).int()
        labels = torch.full_like(cls, -1)
        labels = torch.where(a_max < unmatched, torch.zeros_like(labels), labels)
        labels = torch.where(forced | (a_max >= matched), cls, labels)
        matched_gt = torch.gather(gt[..., :7], 1, a_arg.unsqueeze(-1).expand(-1, -1, 7))
        reg = residual_encode(matched_gt, anchors[None].expand_as(matched_gt))
        reg = torch.where((labels > 0).unsqueeze(-1), reg, torch.zeros_like(reg))
        return labels, reg

    def forward(self, feat, gt):
        cfg = self.cfg
        b = feat.shape[0]
        if KERNEL_GLUE:
            # the three 1x1 convs as one kernel per direction that reads the NCHW map as it stands and writes the position-major outputs
            # (csrc/head1x1.hip); whenever the situation is not the plain one run_heads calls the modules, as below
            cls, box, dirs = _head.run_heads((self.conv_cls, self.conv_box, self.conv_dir_cls), feat)
            cls, box, dirs = cls.reshape(b, -1, 1), box.reshape(b, -1, 7), dirs.reshape(b, -1, cfg.num_dir_bins)
        else:
            cls = self.conv_cls(feat).permute(0, 2, 3, 1).reshape(b, -1, 1)
            box = self.conv_box(feat).permute(0, 2, 3, 1).reshape(b, -1, 7)
            dirs = self.conv_dir_cls(feat).permute(0, 2, 3, 1).reshape(b, -1, cfg.num_dir_bins)
        labels, reg_t = self.assign(gt)
        if cls.is_cuda and cfg.num_dir_bins == 2 and KERNEL_GLUE:
            # the three losses and their logit gradients in one pass (csrc/targets.hip); anchor_losses_tensor_ops states the same
            # in torch ops (and is the CPU path)
            loss = AnchorLossFn.apply(cls.contiguous(), box.contiguous(), dirs.contiguous(), labels.contiguous(), reg_t.contiguous(),
                                      self.anchor_rot, cfg)
        else:
            loss = self.anchor_losses_tensor_ops(cls, box, dirs, labels, reg_t)
        return loss, cls.detach().squeeze(-1), self.decode_proposals(box, dirs)

    def anchor_losses_tensor_ops(self, cls, box, dirs, labels, reg_t):
        cfg = self.cfg
        b = cls.shape[0]
        pos = labels > 0
        norm = pos.sum(1, keepdim=True).float().clamp_min(1.0)
        # classification (anchor_head_template.py:98-131)
        cls_w = ((labels == 0) | pos).float() / norm
        onehot = pos.float().unsqueeze(-1)
        loss_cls = sigmoid_focal(cls, onehot, cls_w).sum() / b * cfg.rpn_w["cls"]
        # localisation with the sin-difference heading encoding (:133-189)
        reg_w = pos.float() / norm
        sin_p = torch.sin(box[..., 6:7]) * torch.cos(reg_t[..., 6:7])
        sin_t = torch.cos(box[..., 6:7]) * torch.sin(reg_t[..., 6:7])
        diff = torch.cat((box[..., :6] - reg_t[..., :6], sin_p - sin_t), dim=-1)
        loss_loc = (smooth_l1(diff, 1.0 / 9.0) * reg_w.unsqueeze(-1)).sum() / b * cfg.rpn_w["loc"]
        # direction bins (:144-157, 191-206)
        rot_gt = reg_t[..., 6] + self.anchors[None, :, 6]
        dir_t = torch.floor(limit_period(rot_gt - cfg.dir_offset, 0, TWO_PI) / (TWO_PI / cfg.num_dir_bins)).long()
        dir_t = dir_t.clamp(0, cfg.num_dir_bins - 1)
        dir_w = pos.float() / pos.float().sum(-1, keepdim=True).clamp_min(1.0)
        loss_dir = (F.cross_entropy(dirs.permute(0, 2, 1), dir_t, reduction="none") * dir_w).sum() / b * cfg.rpn_w["dir"]
        return loss_cls + loss_loc + loss_dir

    def decode_proposals(self, box, dirs):
        """Proposals for the second stage (generate_predicted_boxes, anchor_head_template.py:222-275)."""
        cfg = self.cfg
        with torch.no_grad():
            boxes = residual_decode(box.detach(), self.anchors[None])
            period = TWO_PI / cfg.num_dir_bins
            rot = limit_period(boxes[..., 6] - cfg.dir_offset, cfg.dir_limit_offset, period)
            rot = rot + cfg.dir_offset + period * dirs.detach().argmax(-1).to(boxes.dtype)
            boxes = torch.cat((boxes[..., :6], rot.unsqueeze(-1)), dim=-1)
        return boxes


# ---------------------------------------------------------------- voxel-to-point decoder --------------
class LateralBlock(nn.Module):
    """LateralBottomResBlock (residual_v2p_decoder.py:46-146): 3-NN inverse-distance interpolation of one sparse level
    onto the key points, then relu(net(lateral) + downsample(bottom))."""

    def __init__(self, cfg, stride, lateral_c, bottom_c, out_c):
        super().__init__()
        self.stride, self.cfg = stride, cfg
        bn = dict(eps=1e-3, momentum=0.01)
        if bottom_c > 0:
            self.net = nn.Sequential(nn.Linear(lateral_c, out_c, bias=False), nn.BatchNorm1d(out_c, **bn), nn.ReLU(),
                                     nn.Linear(out_c, out_c, bias=False), nn.BatchNorm1d(out_c, **bn))
            self.downsample = nn.Sequential(nn.Linear(bottom_c, out_c, bias=False), nn.BatchNorm1d(out_c, **bn))
        else:
            self.net = None

    def forward(self, level, bottom, key_xyz, key_cnt):
        cfg = self.cfg
        idx = level.indices
        vs = dconst(idx, tuple(float(v) * self.stride for v in cfg.voxel_size))
        centres = (idx[:, 1:4].flip(-1).float() + 0.5) * vs + dconst(idx, tuple(float(v) for v in cfg.point_cloud_range[:3]))
        # rows of a level are grouped by sample; counted without torch.bincount, which reads the maximum back to the host
        vox_cnt = (idx[:, 0:1] == torch.arange(key_cnt.shape[0], device=idx.device, dtype=idx.dtype)).sum(0, dtype=torch.int32)
        # the known points are voxel centres of pitch vs: a grid of two pitches per cell holds <= 8 of them per cell
        dist, nn_idx = pn2_stack.three_nn(key_xyz, key_cnt, centres.contiguous(), vox_cnt, 2.0 * float(cfg.voxel_size[0]) * self.stride)
        recip = 1.0 / (dist + 1e-8)
        weight = recip / recip.sum(dim=1, keepdim=True)
        lateral = pn2_stack.three_interpolate(level.features, nn_idx, weight)
        if self.net is None:
            return lateral
        return F.relu(run_rows(self.net, lateral) + run_rows(self.downsample, bottom))


class V2PDecoder(nn.Module):
    """ResidualVoxelToPointDecoder (residual_v2p_decoder.py:149-313)."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.decode_block_init = LateralBlock(cfg, cfg.init_stride, cfg.init_channels, -1, cfg.init_channels)
        self.decode_blocks_map = nn.ModuleDict()
        prev = cfg.init_channels
        for name, stride, lat, out in cfg.decode_levels:
            self.decode_blocks_map[name] = LateralBlock(cfg, stride, lat, prev, out)
            prev = out
        self.decode_block_out = nn.Sequential(nn.Linear(prev, cfg.decoder_out, bias=False),
                                              nn.BatchNorm1d(cfg.decoder_out, eps=1e-3, momentum=0.01), nn.ReLU())

    @torch.no_grad()
    def sample_keypoints(self, clouds):
        """Furthest point sampling of every cloud to NUM_KEYPOINTS (:196-232); short clouds repeat their head (:220-222)."""
        m = self.cfg.num_keypoints
        n0 = clouds[0].shape[0]
        if all(c.shape[0] == n0 for c in clouds):
            xyz = torch.stack([c[:, :3] for c in clouds]).contiguous()
            idx = pn2_stack.furthest_point_sample(xyz, m).long()
            per = [(xyz[b], idx[b]) for b in range(len(clouds))]
        elif clouds[0].is_cuda:
            # unequal clouds: one stacked call, the samples side by side (a per-sample loop runs them one after the other on one CU each)
            cnt = [c.shape[0] for c in clouds]
            idx = pn2_stack.stack_furthest_point_sample(torch.cat([c[:, :3] for c in clouds]).contiguous(), cnt, m).long()
            per = [(c[:, :3].contiguous(), idx[b]) for b, c in enumerate(clouds)]
        else:   # CPU tensors (the run on the oracle's backend, which answers the equal-size entry point only)
            per = []
            for c in clouds:
                xyz = c[:, :3].contiguous()
                per.append((xyz, pn2_stack.furthest_point_sample(xyz.unsqueeze(0), m)[0].long()))
        out = []
        for xyz, idx in per:
            n = xyz.shape[0]
            if n < m:
                idx = torch.cat((idx[:n], idx[:m - n]))
            out.append(xyz[idx])
        return torch.stack(out)                                                  # (B, M, 3)

    def start_sampling(self, clouds, wait=True):
        """Enqueues sample_keypoints on a side stream (GPU tensors only); returns a handle for forward().
        wait=False: the clouds are known to be complete (an input pipeline's own buffers) — the side stream is not ordered after
        the calling thread's current stream (a helper thread's current stream is the default one: waiting for it would put the
        sampler behind whatever the training thread has queued)."""
        if not clouds[0].is_cuda:
            return None
        dev = clouds[0].device
        side = side_stream("fps", dev)
        if wait:
            side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            key = self.sample_keypoints(clouds)
        return key, side

    def forward(self, clouds, levels, key_job=None):
        cfg = self.cfg
        if key_job is None:
            key = self.sample_keypoints(clouds)
        else:
            key, side = key_job
            torch.cuda.current_stream(key.device).wait_stream(side)
            key.record_stream(torch.cuda.current_stream(key.device))
        b, m, _ = key.shape
        key_xyz = key.view(-1, 3)
        key_cnt = torch.full((b,), m, dtype=torch.int32, device=key.device)
        x = self.decode_block_init(levels[cfg.init_source], None, key_xyz, key_cnt)
        for name, _, _, _ in cfg.decode_levels:
            x = self.decode_blocks_map[name](levels[name], x, key_xyz, key_cnt)
        return key, run_rows(self.decode_block_out, x)


# ---------------------------------------------------------------- point head ---------------------------
class PointHead(nn.Module):
    """PointHeadSimple (point_head_simple.py, point_head_template.py:47-142): per-point foreground logit, targets from
    points_in_boxes on the boxes and on the boxes enlarged by GT_EXTRA_WIDTH (in between = ignored)."""

    def __init__(self, cfg, cin):
        super().__init__()
        self.cfg = cfg
        self.cls_layers = mlp1d(cin, cfg.point_cls_fc, out=1)

    @torch.no_grad()
    def assign(self, key, gt):
        boxes = gt[..., :7].contiguous()
        ext = boxes.clone()
        ext[..., 3:6] += dconst(boxes, tuple(float(v) for v in self.cfg.gt_extra_width), boxes.dtype)
        # zero-padded rows must stay empty boxes after the enlargement
        ext = torch.where((boxes[..., 3:6].abs().sum(-1, keepdim=True) > 0), ext, boxes)
        inside = roiaware_pool3d_utils.points_in_boxes_gpu(key, boxes) >= 0
        near = roiaware_pool3d_utils.points_in_boxes_gpu(key, ext) >= 0
        labels = inside.long()
        labels.masked_fill_(inside ^ near, -1)
        return labels.view(-1)

    def forward(self, key, feats, gt):
        logits = run_rows(self.cls_layers, feats)                                # (B*M, 1)
        labels = self.assign(key, gt)
        if KERNEL_GLUE and logits.is_cuda and logits.dtype == torch.float32 and logits.shape[1] == 1:
            # loss, logit gradient and score in one pass (csrc/targets.hip); the lines below state the same in tensor ops
            return PointLossFn.apply(logits, labels, self.cfg.point_cls_weight)
        pos = labels > 0
        w = ((labels == 0) | pos).float() / pos.sum().float().clamp_min(1.0)
        loss = sigmoid_focal(logits, pos.float().unsqueeze(-1), w).sum() * self.cfg.point_cls_weight
        return loss, torch.sigmoid(logits).max(dim=-1).values


def rows_linear(x, weight, bias=None):
    """y[r] = x[r] @ weight.T (+ bias) for x (R, N, Cin) and a conv / linear weight (Cout, Cin[, 1, 1]), as a batched product with
    the weight broadcast over R.  The forward is the same GEMM; the point is the weight gradient: autograd then forms it per RoI
    (R products with K = N) and sums over R, instead of one product with K = R * N = 196 608 and a 3 .. 256-wide output, which
    rocBLAS runs at a few TFLOP/s."""
    w = weight.reshape(weight.shape[0], -1).t().unsqueeze(0).expand(x.shape[0], -1, -1)
    y = torch.bmm(x, w)
    return y if bias is None else y + bias


def sa_msg_grid(sa, xyz, features, centres, rows=None):
    """PointnetSAModuleMSG.forward (pointnet2_modules.py:30-62) for the bn=False, use_xyz=True, max-pool module of the RoI head,
    with the first shared-MLP layer taken out of the neighbourhood: it is linear in [xyz_j - c_i ; f_j], so
    W1 [xyz_j - c_i ; f_j] = (W1f f_j + W1x xyz_j) - W1x c_i is one GEMM per POINT (512 per RoI) and one per CENTRE (216) instead
    of one per (centre, sample) pair (216 x 16 / 32); what is grouped is the 64-channel product, not the 131-channel input.
    Same parameters, same result up to fp32 summation order.  xyz (R, N, 3), features (R, C, N) (or `rows` = the same point-major,
    (R, N, C)), centres (R, M, 3) -> (R, sum C_k, M)."""
    outs = []
    xyz_t = xyz.transpose(1, 2)                                                  # (R, 3, N)
    ctr_t = centres.transpose(1, 2)                                              # (R, 3, M)
    for grouper, mlp in zip(sa.groupers, sa.mlps):
        layers = list(mlp)
        w1 = layers[0].weight[:, :, 0, 0]                                        # (C1, 3 + C)
        idx = pn2_batch.ball_query(grouper.radius, grouper.nsample, xyz, centres)
        tail = layers[1:]
        fusable = (len(tail) == 3 and isinstance(tail[0], nn.ReLU) and isinstance(tail[1], nn.Conv2d) and isinstance(tail[2], nn.ReLU)
                   and tail[1].bias is None and tail[1].weight.shape[:2] == (w1.shape[0], w1.shape[0]) and xyz.is_cuda)
        if fusable:
            # rows of 64 channels per point / centre; gather, second layer, ReLU and the max over the samples in one kernel
            if rows is None:
                rows = features.transpose(1, 2).contiguous()                     # point-major (R, N, C)
            per_point = rows_linear(rows, w1[:, 3:]) + rows_linear(xyz, w1[:, :3])                                     # (R, N, C1)
            per_centre = rows_linear(centres, w1[:, :3])                                                               # (R, M, C1)
            if pn2_fused.supported(per_point, idx):
                outs.append(pn2_fused.sa_grid_max(per_point, per_centre, idx, tail[1].weight[:, :, 0, 0]).transpose(1, 2))
                continue
        if features is None:
            features = rows.transpose(1, 2).contiguous()
        per_point = (torch.matmul(w1[:, 3:], features) + torch.matmul(w1[:, :3], xyz_t)).contiguous()   # (R, C1, N)
        per_centre = torch.matmul(w1[:, :3], ctr_t)                              # (R, C1, M)
        h = pn2_batch.grouping_operation(per_point, idx) - per_centre.unsqueeze(-1)                     # (R, C1, M, ns)
        for layer in tail:
            h = layer(h)
        outs.append(h.amax(dim=-1))
    return torch.cat(outs, dim=1)


# ---------------------------------------------------------------- RoI head ------------------------------
class IoUGuidedRoIHead(nn.Module):
    """IoUGuidedRoIHead (iouguided_roi_head.py) + RoIWithIoUHeadTemplate (roi_withiou_head_template.py) +
    ProposalTargetLayer (proposal_target_layer.py), training path."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.bev_grid_pool_layer = bev_grid_pooling.BEVGridPooling(
            type("Cfg", (), dict(IN_CHANNELS=cfg.bev_pool_in, OUT_CHANNELS=cfg.bev_pool_out))(), cfg.point_cloud_range, cfg.voxel_size)
        self.roipoint_pool3d_layer = roipoint_pool3d_utils.RoIPointPool3d(cfg.num_sampled_points, list(cfg.pool_extra_width))
        chans = [5] + list(cfg.xyz_up)
        up = []
        for a, c in zip(chans[:-1], chans[1:]):
            up += [nn.Conv2d(a, c, 1), nn.ReLU()]
        self.xyz_up_layer = nn.Sequential(*up)
        c_out = cfg.xyz_up[-1]
        self.merge_down_layer = nn.Sequential(nn.Conv2d(2 * c_out, c_out, 1), nn.ReLU())
        self.SA_modules = nn.ModuleList([pn2_batch_modules.PointnetSAModuleMSG(
            npoint=cfg.grid_size_roi ** 3, radii=list(cfg.sa_radii), nsamples=list(cfg.sa_nsamples),
            mlps=[[c_out] + list(m) for m in cfg.sa_mlps], use_xyz=True, bn=False)])
        sa_out = sum(m[-1] for m in cfg.sa_mlps)
        g3 = cfg.grid_size_roi ** 3
        layers, pre = [], g3 * (sa_out + cfg.bev_pool_out)
        for k, f in enumerate(cfg.interact_filters):
            layers += [nn.Conv1d(pre, f, 1, bias=False), nn.BatchNorm1d(f), nn.ReLU()]
            if k != len(cfg.interact_filters) - 1 and cfg.dp_ratio > 0:
                layers.append(nn.Dropout(cfg.dp_ratio))
            pre = f
        self.grid_interact_fc_layer = nn.Sequential(*layers)
        up, c = [], 3
        for f in cfg.cge_up:
            up += [nn.Conv2d(c, f, 1, bias=False), nn.BatchNorm2d(f), nn.ReLU()]
            c = f
        inter = []
        for f in cfg.cge_interact:
            inter += [nn.Conv1d(c, f, 8, bias=False), nn.BatchNorm1d(f), nn.ReLU()]
            c = f
        self.cge_up, self.cge_inter = nn.Sequential(*up), nn.Sequential(*inter)
        self.feature_fusion = mlp1d(cfg.interact_filters[-1] + cfg.cge_interact[-1], cfg.fuse_filters, conv=True)
        shared = cfg.fuse_filters[-1]
        self.cls_layers = mlp1d(shared, cfg.cls_fc, out=1, conv=True, dropout_after_first=cfg.dp_ratio)
        self.reg_layers = mlp1d(shared, cfg.reg_fc, out=8, conv=True, dropout_after_first=cfg.dp_ratio)
        for mod in self.modules():
            if isinstance(mod, (nn.Conv1d, nn.Conv2d)):
                nn.init.xavier_normal_(mod.weight)
                if mod.bias is not None:
                    nn.init.constant_(mod.bias, 0)
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)

    # -- proposal layer: top-k + rotated NMS per sample, survivors stay on the device (roi_withiou_head_template.py:46-101)
    @torch.no_grad()
    def proposals(self, scores, boxes):
        cfg = self.cfg
        b = scores.shape[0]
        top_s, top_i = torch.topk(scores, k=min(cfg.nms_pre, scores.shape[1]), dim=1)     # descending: the order NMS wants
        cand = torch.gather(boxes, 1, top_i.unsqueeze(-1).expand(-1, -1, 7)).contiguous()
        if not KERNEL_GLUE:   # the reference's loop: one nms_gpu per sample over all candidates, the cut afterwards (roi_head_template.py:60-85)
            rois, roi_scores = boxes.new_zeros(b, cfg.nms_post, 7), boxes.new_zeros(b, cfg.nms_post)
            # the reference hands nms_gpu its whole NMS_CONFIG as keyword arguments (model_nms_utils.py:14-16); this pcdet.ops stops at
            # NMS_POST_MAXSIZE survivors when it is there.  The reference-structure baseline (refstyle.py) withholds it: its NMS is full.
            kw = {} if FULL_NMS else dict(NMS_TYPE="nms_gpu", NMS_THRESH=cfg.nms_thresh, NMS_PRE_MAXSIZE=cfg.nms_pre, NMS_POST_MAXSIZE=cfg.nms_post)
            for i in range(b):
                sel, _ = iou3d_nms_utils.nms_gpu(cand[i], top_s[i], cfg.nms_thresh, **kw)
                sel = sel[:cfg.nms_post]
                rois[i, :len(sel)], roi_scores[i, :len(sel)] = cand[i][sel], top_s[i][sel]
            return rois, roi_scores
        keep, cnt = iou3d_nms_cuda.nms_batch_device(cand, cfg.nms_thresh, cfg.nms_post)   # the first nms_post survivors per sample
        k = keep.shape[1]
        valid = torch.arange(k, device=boxes.device)[None] < cnt[:, None]
        keep = torch.where(valid, keep, torch.zeros_like(keep))
        rois = boxes.new_zeros(b, cfg.nms_post, 7)
        roi_scores = boxes.new_zeros(b, cfg.nms_post)
        rois[:, :k] = torch.gather(cand, 1, keep.unsqueeze(-1).expand(-1, -1, 7)) * valid.unsqueeze(-1)
        roi_scores[:, :k] = torch.gather(top_s, 1, keep) * valid
        return rois, roi_scores

    # -- ProposalTargetLayer.sample_rois_for_rcnn / subsample_rois (proposal_target_layer.py:92-217) without host round trips
    @torch.no_grad()
    def sample_targets(self, rois, gt, uniforms):
        cfg = self.cfg
        b, r, _ = rois.shape
        n = cfg.roi_per_image
        if rois.is_cuda and KERNEL_GLUE:
            rois, gt = rois.contiguous(), gt.contiguous()
            iou = rois.new_empty(b, r, gt.shape[1])
            with _nat.device_guard(rois.device):   # boxes_iou3d_gpu for the batch in one launch (same float operations)
                _nat.call("fv2p_boxes_iou3d_batch", rois, b, r, gt, gt.shape[1], gt.shape[-1], iou, _nat.stream())
        else:
            iou = torch.stack([iou3d_nms_utils.boxes_iou3d_gpu(rois[i], gt[i, :, :7].contiguous()) for i in range(b)])   # (B, R, G)
        if rois.is_cuda and r <= 1024 and KERNEL_GLUE:
            # one launch for the batch (csrc/targets.hip); the tensor formulation below is its statement in torch ops and what a
            # CPU run takes (tests/test_fv2p_step_gpu.py compares the two bit for bit)
            rois, gt, uniforms = rois.contiguous(), gt.contiguous(), uniforms.contiguous().float()
            s_rois, s_gt = rois.new_empty(b, n, 7), gt.new_empty(b, n, gt.shape[-1])
            s_iou, s_index = rois.new_empty(b, n), torch.empty((b, n), dtype=torch.int32, device=rois.device)
            with _nat.device_guard(rois.device):
                _nat.call("fv2p_roi_sample_targets", iou.contiguous(), rois, gt, uniforms, b, r, gt.shape[1], n, gt.shape[-1],
                          float(min(cfg.reg_fg, cfg.cls_fg)), float(cfg.cls_bg_lo), float(cfg.reg_fg), int(round(cfg.fg_ratio * n)),
                          float(cfg.hard_bg_ratio), s_rois, s_gt, s_iou, s_index, _nat.stream())
            return s_rois, s_gt, s_iou
        return self.sample_targets_tensor_ops(iou, rois, gt, uniforms)

    @torch.no_grad()
    def sample_targets_tensor_ops(self, iou, rois, gt, uniforms):
        cfg = self.cfg
        b, r, _ = rois.shape
        n = cfg.roi_per_image
        max_ov, assign = iou.max(dim=2)
        fg = max_ov >= min(cfg.reg_fg, cfg.cls_fg)
        easy = max_ov < cfg.cls_bg_lo
        hard = (max_ov < cfg.reg_fg) & (max_ov >= cfg.cls_bg_lo)
        n_fg, n_easy, n_hard = fg.sum(1), easy.sum(1), hard.sum(1)
        n_bg = n_easy + n_hard
        u_perm, u_pick = uniforms[:, :r], uniforms[:, r:r + n]

        def compact(mask, keys=None):
            """Row indices of the set members first (in index order, or in random order when keys are given)."""
            k = torch.where(mask, keys if keys is not None else torch.zeros_like(max_ov), torch.full_like(max_ov, 2.0))
            return torch.sort(k, dim=1, stable=True).indices

        fg_order = compact(fg, u_perm)                 # random permutation of the foreground rois, then the rest
        hard_list, easy_list = compact(hard), compact(easy)
        fg_quota = int(round(cfg.fg_ratio * n))
        fg_take = torch.where(n_bg > 0, n_fg.clamp(max=fg_quota), torch.where(n_fg > 0, torch.full_like(n_fg, n), torch.zeros_like(n_fg)))
        bg_take = n - fg_take
        hard_take = torch.where(n_easy > 0, torch.minimum((bg_take.float() * cfg.hard_bg_ratio).long(), n_hard), bg_take)
        hard_take = torch.where(n_hard > 0, hard_take, torch.zeros_like(hard_take))
        slot = torch.arange(n, device=rois.device)[None].expand(b, -1)

        def pick(lst, count):                          # with replacement: floor(u * count)
            j = (u_pick * count[:, None].float()).long().clamp(max=(count[:, None] - 1).clamp_min(0))
            return torch.gather(lst, 1, j)

        only_fg = (n_bg == 0)[:, None]
        fg_sel = torch.where(only_fg, pick(fg_order, n_fg), torch.gather(fg_order, 1, slot.clamp(max=r - 1)))
        sel = torch.where(slot < fg_take[:, None], fg_sel,
                          torch.where(slot < (fg_take + hard_take)[:, None], pick(hard_list, n_hard), pick(easy_list, n_easy)))
        g7 = lambda t, idx, w: torch.gather(t, 1, idx.unsqueeze(-1).expand(-1, -1, w))
        s_rois = g7(rois, sel, 7)
        s_iou = torch.gather(max_ov, 1, sel)
        s_gt = g7(gt, torch.gather(assign, 1, sel), gt.shape[-1])
        return s_rois, s_gt, s_iou

    @staticmethod
    def canonical_targets(rois, gt_of_rois):
        """RoIWithIoUHeadTemplate.assign_targets (:103-135): gt boxes in the roi's frame, heading folded to [-pi/2, pi/2]."""
        b, n, _ = rois.shape
        ry = rois[..., 6] % TWO_PI
        g = gt_of_rois.clone()
        g[..., 0:3] -= rois[..., 0:3]
        g[..., 6] -= ry
        g = rotate_z(g.view(-1, 1, g.shape[-1]), -ry.view(-1)).view(b, n, -1)
        h = g[..., 6] % TWO_PI
        opp = (h > math.pi * 0.5) & (h < math.pi * 1.5)
        h = torch.where(opp, (h + math.pi) % TWO_PI, h)
        h = torch.where(h > math.pi, h - TWO_PI, h).clamp(-math.pi / 2, math.pi / 2)
        return torch.cat((g[..., :6], h.unsqueeze(-1), g[..., 7:]), dim=-1)

    def pool_points(self, key, feats, scores, rois):
        """roipool3d_gpu (:144-195): 512 points per enlarged roi with [score, depth, features], in the roi's frame."""
        if KERNEL_GLUE and key.is_cuda and feats.dtype == torch.float32:
            # the pool kernel writes the rows in the roi's frame itself (csrc/roi_pool.hip); the lines below state the same in tensor ops
            return pool_points_in_frame(self.roipoint_pool3d_layer, self.cfg.depth_normalizer, key, feats, scores, rois)
        b = key.shape[0]
        depth = key.view(-1, 3).norm(dim=1) / self.cfg.depth_normalizer - 0.5
        allf = torch.cat((scores.detach()[:, None], depth[:, None], feats), dim=1).view(b, -1, feats.shape[1] + 2)
        pooled, empty = self.roipoint_pool3d_layer(key, allf, rois)
        # the pool itself carries no gradient (reference: under no_grad), neither does what follows here
        pooled = pooled.detach()
        with torch.no_grad():
            pooled[..., 0:3] -= rois[:, :, None, 0:3]
            pooled = pooled.view(-1, pooled.shape[-2], pooled.shape[-1])
            pooled[..., 0:3] = rotate_z(pooled[..., 0:3], -rois.reshape(-1, 7)[:, 6])
            pooled[empty.view(-1) > 0] = 0
        return pooled

    def grid_points(self, rois):
        g = self.cfg.grid_size_roi
        r = rois.reshape(-1, 7)
        ii = torch.arange(g, device=r.device, dtype=torch.float32)
        cell = torch.stack(torch.meshgrid(ii, ii, ii, indexing="ij"), dim=-1).view(1, -1, 3)       # nonzero() order: x slowest
        local = (cell + 0.5) / g * r[:, None, 3:6] - r[:, None, 3:6] / 2
        world = rotate_z(local, r[:, 6]) + r[:, None, 0:3]
        return world, local

    def prepare(self, bev, prop_scores, prop_boxes, gt, uniforms):
        """Everything of the second stage that needs no key points: proposals, target sampling, the RoI grids, the BEV stream and
        the corner-geometry stream.  The detector runs it before it joins the key-point sampling stream."""
        b = bev.shape[0]
        rois, _ = self.proposals(prop_scores, prop_boxes)
        s_rois, s_gt, s_iou = self.sample_targets(rois, gt, uniforms)
        # fv2p_roi_loss forms the canonical targets itself: on that route nothing reads gt_ct (see losses)
        gt_ct = None if (KERNEL_GLUE and s_rois.is_cuda) else self.canonical_targets(s_rois, s_gt)
        return dict(rois=rois, s_rois=s_rois, s_gt=s_gt, s_iou=s_iou, gt_ct=gt_ct, **self.roi_streams(bev, s_rois))

    def roi_streams(self, bev, s_rois, bev_stride=8):
        """The two streams of forward_single_loop (iouguided_roi_head.py:223-304) that need no key points: the RoI grids with the BEV
        features gathered at them, and the corner-geometry embedding."""
        b = bev.shape[0]
        g = self.cfg.grid_size_roi
        kernel = KERNEL_GLUE and s_rois.is_cuda and s_rois.dtype == torch.float32 and not s_rois.requires_grad
        if kernel:   # local grid, world column points and corner offsets from one launch (csrc/targets.hip: fv2p_roi_grid)
            local, column, corners = roi_grid_geometry(s_rois, g)
        else:
            world, local = self.grid_points(s_rois)
            column = world.view(world.shape[0], g * g, g, 3)[:, :, 0] if KERNEL_GLUE and world.shape[1] == g ** 3 else None
        n_roi = local.shape[0]
        # BEV stream: bilinear gather at the grid points + channel compression (:243-255).  The g grid points of a column (same x
        # and y index, z fastest: grid_points) share their BEV position — the rotation is about z — so the reference's g^3 gathers
        # per RoI are g^2 different ones: gathered and compressed once per column and broadcast over z (autograd sums the g
        # gradients of a column before the scatter: 6 x fewer float atomics into the map, 6 x fewer rows through the Linear +
        # BatchNorm1d of the compression — whose batch statistics are those of the repeated rows; only the n / (n - 1) factor of its
        # running variance sees 13 824 instead of 82 944 rows).  Values equal the per-point form to rounding (tested).
        batch_dict = {"batch_size": b, "spatial_features_before_head": bev, "spatial_features_stride": bev_stride}
        if column is not None:
            g_bev = self.bev_grid_pool_layer(batch_dict, column.reshape(b, -1, 3))
            g_bev = g_bev.view(n_roi, g * g, 1, -1).expand(-1, -1, g, -1).reshape(n_roi, g ** 3, -1)
        else:
            g_bev = self.bev_grid_pool_layer(batch_dict, world.view(b, -1, 3)).view(world.shape[0], world.shape[1], -1)
        g_bev = g_bev.permute(0, 2, 1).contiguous()
        # corner geometry stream (feature_adaptor/nn_modules.py:6-60): roi-frame corners without rotation or centre
        if not kernel:
            t = dconst(s_rois, _CORNER_SIGNS, s_rois.dtype) / 2
            corners = s_rois.reshape(-1, 7)[:, None, 3:6] * t[None]
        cge = self.cge_inter(self.cge_up(corners.transpose(1, 2).unsqueeze(3).contiguous()).squeeze(-1))
        return dict(local=local, g_bev=g_bev, cge=cge)

    def finish(self, key, feats, scores, prep):
        rois = prep["s_rois"]
        cls, reg = self.predict(key, feats, scores, rois, prep)
        if KERNEL_GLUE and cls.is_cuda:   # the whole [iou, 7 residuals] row: one gradient tensor back, no slices to re-assemble
            loss = self.losses(rois, prep["s_gt"], prep["gt_ct"], prep["s_iou"], cls, reg, None)
        else:
            loss = self.losses(rois, prep["s_gt"], prep["gt_ct"], prep["s_iou"], cls, reg[:, 1:], reg[:, :1])
        return loss, {"rois": prep["rois"], "sampled_rois": rois, "roi_iou": prep["s_iou"]}

    def predict(self, key, feats, scores, rois, prep):
        """forward_single_loop (iouguided_roi_head.py:223-304) from the pooled points on: -> (rcnn_cls (B*n, 1), [iou, 7 residuals] (B*n, 8))."""
        pooled = self.pool_points(key, feats, scores, rois)                                        # (B*n, 512, 5 + C)
        # xyz_up_layer / merge_down_layer are 1x1 convs over the 512 pooled points of each RoI (:223-236): applied point-major, as
        # batched row products (same weights; see rows_linear) - the pooled tensor already is (RoI, point, channel)
        h = pooled[..., 0:5]
        for layer in self.xyz_up_layer:
            h = rows_linear(h, layer.weight, layer.bias) if isinstance(layer, nn.Conv2d) else layer(h)
        h = torch.cat((h, pooled[..., 5:]), dim=2)
        for layer in self.merge_down_layer:
            h = rows_linear(h, layer.weight, layer.bias) if isinstance(layer, nn.Conv2d) else layer(h)
        # point stream: multi-scale ball query around the grid points (:258-275)
        g_pt = sa_msg_grid(self.SA_modules[0], pooled[..., 0:3].contiguous(), None, prep["local"].contiguous(), rows=h)
        grid = torch.cat((g_pt, prep["g_bev"]), dim=1)
        pc = self.grid_interact_fc_layer(grid.view(grid.shape[0], -1, 1))
        shared = self.feature_fusion(torch.cat((pc, prep["cge"]), dim=1))
        cls = self.cls_layers(shared).squeeze(-1)                                                  # (B*n, 1)
        reg = self.reg_layers(shared).squeeze(-1)                                                  # (B*n, 8): [iou, 7 residuals]
        return cls, reg

    @staticmethod
    def reg_losses(rois, gt_src, gt_ct, fg, reg):
        """get_box_reg_layer_loss (roi_withiou_head_template.py:133-195): smooth-L1 (beta 1/9) on the ResidualCoder targets of the
        canonical boxes against the size-only roi anchor, and the corner regularisation of the boxes decoded back into the
        LiDAR frame; both averaged over the foreground rois (fg: (B*n,) 0/1).  Returns (loss_reg, loss_corner)."""
        n_fg = fg.sum().clamp_min(1.0)
        r7 = rois.reshape(-1, 7)
        anchor = torch.cat((torch.zeros_like(r7[:, :3]), r7[:, 3:6], torch.zeros_like(r7[:, 6:7])), dim=1)
        target = residual_encode(gt_ct.reshape(-1, gt_ct.shape[-1])[:, :7], anchor)
        loss_reg = (smooth_l1(reg - target, 1.0 / 9.0) * fg[:, None]).sum() / n_fg
        # corner regularisation over the foreground rois (mean over them == masked sum / count)
        local = residual_decode(reg, anchor)
        world = rotate_z(local.unsqueeze(1), r7[:, 6]).squeeze(1)
        world = torch.cat((world[:, :3] + r7[:, :3], world[:, 3:6], world[:, 6:7] + r7[:, 6:7]), dim=1)   # decoded against the roi's heading
        g = gt_src.reshape(-1, gt_src.shape[-1])[:, :7]
        loss_corner = (corner_loss_lidar(world, g) * fg).sum() / n_fg
        return loss_reg, loss_corner

    def losses(self, rois, gt_src, gt_ct, iou, cls, reg, iou_pred):
        """get_box_cls_layer_loss / get_box_reg_layer_loss / get_box_iouscore_layer_loss (:137-265), CLS_SCORE_TYPE roi_iou.
        iou_pred None: reg holds the whole (R, 8) row [iou, 7 residuals].  gt_ct None: the canonical targets are formed here."""
        cfg = self.cfg
        if KERNEL_GLUE and cls.is_cuda and cls.dtype == torch.float32:
            # losses and logit gradients in one launch (csrc/targets.hip: fv2p_roi_loss); the lines below state the same in tensor ops
            return RoiLossFn.apply(rois, gt_src, iou, cls, reg if iou_pred is None else torch.cat((iou_pred, reg), dim=1), cfg)
        if iou_pred is None:
            reg, iou_pred = reg[:, 1:], reg[:, :1]
        if gt_ct is None:
            gt_ct = self.canonical_targets(rois.reshape(1, -1, 7), gt_src.reshape(1, -1, gt_src.shape[-1]))
        iou = iou.view(-1)
        soft = ((iou - cfg.cls_bg) / (cfg.cls_fg - cfg.cls_bg)).clamp(0, 1)     # 1 above fg, 0 below bg, linear in between
        soft = torch.where(iou > cfg.cls_fg, torch.ones_like(soft), torch.where(iou < cfg.cls_bg, torch.zeros_like(soft), soft))
        loss_cls = F.binary_cross_entropy(torch.sigmoid(cls.view(-1)), soft, reduction="none").mean()   # every label >= 0
        fg = (iou > cfg.reg_fg).float()
        loss_reg, loss_corner = self.reg_losses(rois, gt_src, gt_ct, fg, reg)
        # IoU score head: smooth-l1 on the rois above REG_FG_THRESH, labels renormalised to [-1, 1]
        lab = (iou - 0.5) * 2
        valid = (lab >= (cfg.reg_fg - 0.5) * 2).float()
        loss_iou = (F.smooth_l1_loss(iou_pred.view(-1), lab, reduction="none") * valid).sum() / valid.sum().clamp_min(1.0)
        return loss_cls + loss_reg + loss_corner + loss_iou

    def forward(self, key, feats, point_scores, bev, prop_scores, prop_boxes, gt, uniforms):
        return self.finish(key, feats, point_scores, self.prepare(bev, prop_scores, prop_boxes, gt, uniforms))


# ---------------------------------------------------------------- the detector -------------------------
SAFE_FIRST_STEPS = 2   # GPU steps a detector takes on the calling stream only before any side-stream arrangement (MIOpen's first-call search)


class FV2PDetector(nn.Module):
    """FromVoxelToPoint (detectors/fv2p.py): forward returns the summed training loss of the three heads."""

    def __init__(self, cfg=FV2PConfig):
        super().__init__()
        self.cfg = cfg
        self.backbone_3d = VoxelResBackBone8x(cfg.num_point_features, list(cfg.grid_size))
        self.backbone_2d = BEVBackbone(cfg, 256)
        self.dense_head = AnchorHead(cfg, self.backbone_2d.num_bev_features)
        self.post_pfe = V2PDecoder(cfg)
        self.point_head = PointHead(cfg, cfg.decoder_out)
        self.roi_head = IoUGuidedRoIHead(cfg)
        self.taps = None    # set to a dict to collect intermediate results (parity tests)
        self._gpu_steps = 0   # forward passes taken on a GPU so far (the side-stream guard of forward())

    def forward(self, clouds, voxel_features, voxel_coords, gt_boxes, uniforms, key_job=None):
        """clouds: list of (N_b, 4) point tensors; voxel_features / voxel_coords: MeanVFE output + (b, z, y, x) coords of
        the same clouds; gt_boxes (B, G, 8) zero padded; uniforms (B, nms_post + roi_per_image) in [0, 1).
        key_job: handle of post_pfe.start_sampling(clouds) when the caller has enqueued the key-point sampling of this batch
        already (it needs the raw points only, so an input pipeline can run it during the step before)."""
        b = len(clouds)
        # The first calls of every dense conv shape run MIOpen's solver search; with a branch of the step on a side stream that search
        # hung the device queue on one fresh box in three (never once the results were cached: DESIGN.md 1).  Whoever asks for a
        # side-stream arrangement therefore gets the detector's first SAFE_FIRST_STEPS GPU steps with both BRANCHES on the calling stream,
        # then the arrangement asked for (FV2P_SAFE_FIRST=0 switches the guard off).  The guard covers the dense / point branch streams, whose
        # kernels are MIOpen's; key-point sampling (this library's kernel only) keeps its own stream from the first step on.  Counted per
        # detector, not per process: the search is per conv SHAPE, and a second detector may bring new shapes.  bench.py takes the guarded
        # steps untimed when its warm-up is shorter (`guard_steps`); tests/test_fv2p_step_gpu.py::test_stream_arrangements_give_the_same_step
        # holds the side-stream arrangement to the single-stream step that the oracle comparison runs.
        on_gpu = clouds[0].is_cuda
        branch_streams = on_gpu and self._gpu_steps >= (0 if os.environ.get("FV2P_SAFE_FIRST") == "0" else SAFE_FIRST_STEPS)
        if on_gpu:
            self._gpu_steps += 1
        # key-point sampling needs the raw points only: it runs beside the two backbones on its own stream (three workgroups
        # for 16 k dependent rounds) and is joined where the decoder starts
        if key_job is None and self.cfg.key_stream:
            key_job = self.post_pfe.start_sampling(clouds)
        out, levels = self.backbone_3d(voxel_features, voxel_coords, b)
        if self.cfg.dense_branch_stream and branch_streams:
            # From here the step has two independent branches until the RoI head's `finish`: the dense one (HeightCompression, BEV
            # backbone, anchor head, second-stage preparation: large MIOpen kernels) on a side stream, and decoder + point head
            # (~150 small kernels) on the calling stream; autograd replays each on its stream in the backward pass, where the
            # dense convolutions' gradients overlap the point branch again.  (The mirror arrangement — point branch on a side
            # stream started right after the sparse backbone — hung the device queue in every second run; it remains below in its
            # safe form, started after the preparation, for cfg.dense_branch_stream = False.)
            dev = clouds[0].device
            side, main = side_stream("dense", dev), torch.cuda.current_stream(dev)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                bev, loss_rpn, prop_scores, prop_boxes = self.dense_branch(out, b, gt_boxes)
                prep = self.roi_head.prepare(bev, prop_scores, prop_boxes, gt_boxes, uniforms)
            key, point_feats = self.post_pfe(clouds, levels, key_job)
            loss_point, point_scores = self.point_head(key, point_feats, gt_boxes)
            main.wait_stream(side)
            for t in [bev, loss_rpn, prop_scores, prop_boxes] + [v for v in prep.values() if torch.is_tensor(v)]:
                t.record_stream(main)
        else:
            bev, loss_rpn, prop_scores, prop_boxes = self.dense_branch(out, b, gt_boxes)
            prep = self.roi_head.prepare(bev, prop_scores, prop_boxes, gt_boxes, uniforms)   # still no key points needed
            branch = self.point_branch_start(clouds, levels, key_job, gt_boxes, branch_streams and not self.cfg.dense_branch_stream)
            key, point_feats, loss_point, point_scores = self.point_branch_join(branch)
        loss_rcnn, aux = self.roi_head.finish(key, point_feats, point_scores, prep)
        if self.taps is not None:
            self.taps.update(keypoints=key, point_features=point_feats, point_scores=point_scores, bev=bev, prop_boxes=prop_boxes,
                             prop_scores=prop_scores, loss_rpn=loss_rpn, loss_point=loss_point, loss_rcnn=loss_rcnn, **aux)
        return loss_rpn + loss_point + loss_rcnn

    def dense_branch(self, out, b, gt_boxes):
        if getattr(self, "bev_channels_last", False):
            spatial = BEVBackbone.height_compression(out).contiguous(memory_format=torch.channels_last)
        else:
            spatial = out   # HeightCompression (height_compression.py:10-26) is the BEV backbone's: its first conv may not need the map
        bev = self.backbone_2d(spatial)
        loss_rpn, prop_scores, prop_boxes = self.dense_head(bev, gt_boxes)
        return bev, loss_rpn, prop_scores, prop_boxes

    def point_branch_start(self, clouds, levels, key_job, gt_boxes, allowed=True):
        """Decoder + point head.  Their only gradient is the point loss (the RoI head pools the point features under no_grad), so
        in backward this chain of ~150 small kernels is independent of the BEV / anchor / RoI chain until both reach the sparse
        backbone.  Run on its own stream in the forward pass, autograd replays it on that stream in the backward pass, beside the
        dense convolutions' gradients on the main stream."""
        if not (allowed and self.cfg.point_branch_stream and clouds[0].is_cuda and key_job is not None):
            key, feats = self.post_pfe(clouds, levels, key_job)
            loss, scores = self.point_head(key, feats, gt_boxes)
            return (key, feats, loss, scores), None
        dev = clouds[0].device
        side = side_stream("point", dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            key, feats = self.post_pfe(clouds, levels, key_job)
            loss, scores = self.point_head(key, feats, gt_boxes)
        return (key, feats, loss, scores), side

    def point_branch_join(self, branch):
        outs, side = branch
        if side is not None:
            main = torch.cuda.current_stream(outs[0].device)
            main.wait_stream(side)
            for t in outs:
                t.record_stream(main)
        return outs


def pad_gt_boxes(box_lists, device, max_gt=None):
    """[(G_b, 7) numpy] -> (B, G, 8) float32 tensor, class id 1 (Car) in the last column, zero rows as padding
    (dataset.collate_batch, pcdet/datasets/dataset.py:165-171)."""
    g = max_gt or max(len(x) for x in box_lists)
    out = np.zeros((len(box_lists), g, 8), dtype=np.float32)
    for i, bx in enumerate(box_lists):
        k = min(len(bx), g)
        out[i, :k, :7] = bx[:k]
        out[i, :k, 7] = 1.0
    return torch.from_numpy(out).to(device)
