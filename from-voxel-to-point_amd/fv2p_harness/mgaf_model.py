"""Replay of the MGAF-3DSSD detector (BASELINE configs[3]: mgaf-3dssd_3classes.yaml) as a consumer of this repo's `pcdet.ops`:
VoxelResBackBone8x -> HeightCompression -> DCNBEVBackbone (three levels, one MdeformConvBlock per level,
pcdet/models/backbones_2d/dcn_bev_backbone.py:10-132) -> CenterAFHeadSingle (shared conv, modulated deformable feature
adaption with four deformable groups, seven convolutional heads with the segmentation-guided attention,
pcdet/models/dense_heads/center_af_head_single.py:8-148) -> the head's target assignment (CenterTargetAssigner,
keypoint_assigner/centertarget_assigner.py:24-209) and its eight loss terms (center_af_head_template.py:193-460).

Target assignment: the reference draws the maps on the HOST (numpy + cv2, one sample at a time, gt boxes copied to the host and
the maps back: centertarget_assigner.py:41, 72-82); `center_targets` states the same rule as batch tensor ops on the boxes'
device — no host round trip.  Gaussian heat-map, indices, masks and regression targets follow the reference's float64 / float32
arithmetic operation for operation (pinned by tests/golden/pyref_center_targets.npz, written from the reference class); the
segmentation map is cv2.fillConvexPoly in the reference, a library this image lacks: it is restated as "pixel centre inside the
closed quadrilateral, or on one of its 8-connected edge lines" (OpenCV falls back from LINE_AA to 8-connected lines on non-8-bit
images) and is the one target that is NOT pinned.  The per-pixel height map the assigner also returns feeds no loss
(center_af_head_template.py:263-278 reads the per-object target) and is not produced."""
from functools import partial

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from pcdet.ops.DeformableConvolutionV2PyTorch.modules.mdeformable_conv_block import MdeformConvBlock
from pcdet.ops.DeformableConvolutionV2PyTorch.modules.modulated_deform_conv import ModulatedDeformConv

from pcdet.ops.iou3d_nms import iou3d_nms_cuda, iou3d_nms_utils

import fv2p_native as _nat

from .backbone import VoxelResBackBone8x
from .fv2p_model import box_corners, run_maps, sigmoid_focal


class MGAFConfig:
    grid_size = (1408, 1600, 40)
    num_point_features = 4
    layer_nums, layer_strides, num_filters = (5, 5, 5), (1, 2, 2), (128, 256, 256)
    upsample_strides, num_upsample_filters = (1, 2, 4), (256, 256, 256)
    shared_fc = (256,)
    head_deformable_groups = 4
    heads = (("hm", 3), ("offset", 2), ("height", 1), ("dim", 3), ("rot", 24), ("segm", 1), ("iouscore", 1))   # 3 classes
    head_conv = 128
    # TARGET_ASSIGNER_CONFIG / LOSS_CONFIG of mgaf-3dssd_3classes.yaml:134-175
    point_cloud_range = (0.0, -40.0, -3.0, 70.4, 40.0, 1.0)
    voxel_size = (0.05, 0.05, 0.1)
    feature_map_stride, gaussian_minoverlap, gaussian_minradius, max_objs = 8, 0.01, 2, 50
    num_iouscore_training_samples = 24
    loss_weights = dict(hm=1.0, offset=1.0, height=1.0, dim=1.0, rot=1.0, segm=1.0, corner=1.0, iouscore=1.0)
    rot_bins, iou_fg_thresh, iou_bg_thresh = 12, 0.75, 0.25
    # test time: NUM_INFERENCE_SAMPLES of the dense head and POST_PROCESSING of mgaf-3dssd_3classes.yaml
    num_inference_samples = 50
    score_thresh, nms_thresh, nms_pre_maxsize, nms_post_maxsize = 0.501, 0.1, 4096, 500


class DCNBEVBackbone(nn.Module):
    def __init__(self, cfg, cin):
        super().__init__()
        bn = partial(nn.BatchNorm2d, eps=1e-3, momentum=0.01)
        self.blocks, self.deblocks = nn.ModuleList(), nn.ModuleList()
        for n, s, f, us, uf in zip(cfg.layer_nums, cfg.layer_strides, cfg.num_filters, cfg.upsample_strides, cfg.num_upsample_filters):
            seq = [nn.ZeroPad2d(1), nn.Conv2d(cin, f, 3, stride=s, padding=0, bias=False), bn(f), nn.ReLU()]
            for _ in range(n):
                seq += [nn.Conv2d(f, f, 3, padding=1, bias=False), bn(f), nn.ReLU()]
            self.blocks.append(nn.Sequential(*seq))
            self.deblocks.append(nn.Sequential(MdeformConvBlock(f, f, deformable_groups=1), bn(f), nn.ReLU(),
                                               nn.ConvTranspose2d(f, uf, us, stride=us, bias=False), bn(uf), nn.ReLU()))
            cin = f
        self.num_bev_features = sum(cfg.num_upsample_filters)

    def forward(self, x):
        ups = []
        from .fv2p_model import BEVBackbone
        for blk, de in zip(self.blocks, self.deblocks):
            x = BEVBackbone._block(blk, x)   # the leading ZeroPad2d + Conv2d pair as one zero-padded convolution (same sums, no padded copy)
            ups.append(run_maps(de, x))
        return torch.cat(ups, dim=1)


class FeatureAdaption(nn.Module):
    """feature_adaptor/mdeformable_convs.py:14-78: offsets and masks from a plain conv, DCNv2, ReLU."""

    def __init__(self, channels, deformable_groups):
        super().__init__()
        self.conv_offset_mask = nn.Conv2d(channels, deformable_groups * 27, 3, padding=1, bias=True)
        self.conv_adaption = ModulatedDeformConv(channels, channels, stride=1, kernel_size=3, padding=1, deformable_groups=deformable_groups, bias=False)

    def forward(self, x):
        o1, o2, mask = torch.chunk(self.conv_offset_mask(x), 3, dim=1)
        return torch.relu(self.conv_adaption(x, torch.cat((o1, o2), dim=1), torch.sigmoid(mask)))


class CenterAFHead(nn.Module):
    def __init__(self, cfg, cin):
        super().__init__()
        layers, pre = [], cin
        for f in cfg.shared_fc:
            layers += [nn.Conv2d(pre, f, 3, padding=1, bias=False), nn.BatchNorm2d(f), nn.ReLU()]
            pre = f
        self.shared_conv_layer = nn.Sequential(*layers)
        self.feature_adapt = FeatureAdaption(pre, cfg.head_deformable_groups)
        self.heads = nn.ModuleDict({name: nn.Sequential(nn.Conv2d(pre, cfg.head_conv, 3, padding=1, bias=False),
                                                        nn.BatchNorm2d(cfg.head_conv, eps=1e-3, momentum=0.01), nn.ReLU(),
                                                        nn.Conv2d(cfg.head_conv, out, 1, bias=True)) for name, out in cfg.heads})

    def forward(self, x):
        x = self.feature_adapt(run_maps(self.shared_conv_layer, x))
        segm = run_maps(self.heads["segm"], x)
        att = x + torch.sigmoid(segm.detach()).expand_as(x) * x       # mask-guided attention (center_af_head_single.py:84-92)
        preds = {"segm": segm}
        for name, head in self.heads.items():
            if name != "segm":
                preds[name] = run_maps(head, att)
        return preds


# ---------------------------------------------------------------- target assignment ---------------------------------------------------
def gaussian_radius(h, w, min_overlap):
    """center_utils.gaussian_radius (:98-122) on float64 tensors."""
    b1 = h + w
    c1 = w * h * (1 - min_overlap) / (1 + min_overlap)
    r1 = (b1 - torch.sqrt(b1 ** 2 - 4 * c1)) / 2
    b2 = 2 * (h + w)
    c2 = (1 - min_overlap) * w * h
    r2 = (b2 - torch.sqrt(b2 ** 2 - 16 * c2)) / 8
    a3 = 4 * min_overlap
    b3 = -2 * min_overlap * (h + w)
    c3 = (min_overlap - 1) * w * h
    r3 = (b3 + torch.sqrt(b3 ** 2 - 4 * a3 * c3)) / (2 * a3)
    return torch.minimum(torch.minimum(r1, r2), r3)


@torch.no_grad()
def center_targets(gt, cfg, num_classes):
    """CenterTargetAssigner.assign_targets (centertarget_assigner.py:24-209) for the batch, on gt's device.
    gt (B, M, 8) zero padded [x, y, z, dx, dy, dz, heading, class] -> dict with the reference's keys:
    hm_target (B, C, H, W), anno_box_target (B, K, 7), ind_target (B, K) int64, mask_target (B, K) uint8, segm_target (B, 1, H, W),
    src_box_target (B, K, 7), xsys_target (B, K, 2), batch_gtboxes_src (B, M, 8).  K = MAX_OBJS; object k of a sample is its k-th box."""
    dev, b, m = gt.device, gt.shape[0], gt.shape[1]
    k = cfg.max_objs
    lo = torch.tensor(cfg.point_cloud_range[:3], dtype=torch.float32, device=dev)
    hi = torch.tensor(cfg.point_cloud_range[3:], dtype=torch.float32, device=dev)
    vs = torch.tensor(cfg.voxel_size, dtype=torch.float64, device=dev)
    stride = cfg.feature_map_stride
    sy = int(round((cfg.point_cloud_range[4] - cfg.point_cloud_range[1]) / cfg.voxel_size[1] / stride))
    sx = int(round((cfg.point_cloud_range[3] - cfg.point_cloud_range[0]) / cfg.voxel_size[0] / stride))
    boxes = gt[:, :, :7]
    # the reference cuts the trailing all-zero rows (rows whose seven numbers SUM to zero, :50-53) and takes the first K of the rest
    nonzero = boxes.sum(-1) != 0
    pos = torch.arange(m, device=dev)
    last = torch.where(nonzero, pos, torch.zeros_like(pos)).amax(1)                       # cnt of :50-52 (row 0 always stays)
    kk = min(k, m)
    bx = boxes[:, :kk]
    live = (pos[:kk][None] <= last[:, None])
    cls = gt[:, :kk, 7].to(torch.int8).long() - 1                                        # astype(np.int8) then - 1 (:56, 126)
    dimx = bx[..., 3].double() / vs[0] / stride                                          # float32 box / float64 voxel size (:127-128)
    dimy = bx[..., 4].double() / vs[1] / stride
    ok = live & (dimx > 0) & (dimy > 0)
    radius = gaussian_radius(torch.ceil(dimx), torch.ceil(dimy), cfg.gaussian_minoverlap)
    radius = torch.where(ok, radius, torch.zeros_like(radius)).nan_to_num(0.0).clamp(min=0).long().clamp(min=cfg.gaussian_minradius)   # max(int(r), minradius)
    cx = (bx[..., 0] - lo[0]).double() / vs[0] / stride                                  # float32 subtraction, float64 division (:138-139)
    cy = (bx[..., 1] - lo[1]).double() / vs[1] / stride
    cxi, cyi = torch.round(cx).long(), torch.round(cy).long()                            # np.around: half to even, as torch.round
    ok = ok & (cxi >= 0) & (cxi < sx) & (cyi >= 0) & (cyi < sy)
    # heat map: element-wise maximum of the objects' Gaussians, float64 values rounded to float32 once (:160, center_utils.py:139-155)
    ys = torch.arange(sy, device=dev).view(1, 1, sy, 1)
    xs = torch.arange(sx, device=dev).view(1, 1, 1, sx)
    dy, dx = ys - cyi[..., None, None], xs - cxi[..., None, None]
    r = radius[..., None, None]
    sigma = (2 * radius + 1).double()[..., None, None] / 6
    g = torch.exp(-(dx * dx + dy * dy).double() / (2 * sigma * sigma))
    g = torch.where(g < torch.finfo(torch.float64).eps, torch.zeros_like(g), g)          # h[h < eps * h.max()] = 0, h.max() = 1
    g = torch.where((dx.abs() <= r) & (dy.abs() <= r) & ok[..., None, None], g, torch.zeros_like(g)).float()
    hm = gt.new_zeros(b, num_classes, sy, sx)
    for c in range(num_classes):
        hm[:, c] = torch.where((cls == c)[..., None, None], g, torch.zeros_like(g)).amax(1)
    okf = ok.unsqueeze(-1)
    ind = torch.where(ok, sx * cyi + cxi, torch.zeros_like(cxi))
    anno = torch.cat(((cx - cxi).float().unsqueeze(-1), (cy - cyi).float().unsqueeze(-1), bx[..., 2:7]), -1) * okf
    xsys = torch.stack((cxi, cyi), -1).float() * okf
    src = bx * okf
    # segmentation map: the BEV quadrilateral of every live object (corners 0..3 of boxes_to_corners_3d, clipped to the range, in
    # map pixels, rounded to integers :181-190), filled as cv2.fillConvexPoly(lineType 8) does — see the module docstring
    corners = box_corners(bx.reshape(-1, 7)).view(b, kk, 8, 3)[:, :, :4, :2]
    qx = torch.round((corners[..., 0].clamp(lo[0], hi[0]) - lo[0]).double() / vs[0] / stride).long()     # (B, K, 4)
    qy = torch.round((corners[..., 1].clamp(lo[1], hi[1]) - lo[1]).double() / vs[1] / stride).long()
    px, py = xs.view(1, 1, 1, sx), ys.view(1, 1, sy, 1)
    inside_pos = torch.ones(b, kk, sy, sx, dtype=torch.bool, device=dev)
    inside_neg = torch.ones_like(inside_pos)
    on_edge = torch.zeros_like(inside_pos)
    for e in range(4):
        x0, y0 = qx[..., e, None, None], qy[..., e, None, None]
        x1, y1 = qx[..., (e + 1) % 4, None, None], qy[..., (e + 1) % 4, None, None]
        ex, ey = x1 - x0, y1 - y0
        cross = ex * (py - y0) - ey * (px - x0)
        inside_pos &= cross >= 0
        inside_neg &= cross <= 0
        # 8-connected line: one pixel per step of the major axis, the minor coordinate rounded to the nearest row / column
        xmajor = ex.abs() >= ey.abs()
        in_x = (px >= torch.minimum(x0, x1)) & (px <= torch.maximum(x0, x1))
        in_y = (py >= torch.minimum(y0, y1)) & (py <= torch.maximum(y0, y1))
        near_x = (2 * (cross.abs()) <= ex.abs()) & in_x & (ex != 0)       # |py - yline(px)| <= 1/2  <=>  2 |cross| <= |ex|
        near_y = (2 * (cross.abs()) <= ey.abs()) & in_y & (ey != 0)
        point = (ex == 0) & (ey == 0) & (px == x0) & (py == y0)
        on_edge |= torch.where(xmajor, near_x, near_y) | point
    segm = (((inside_pos | inside_neg | on_edge) & ok[..., None, None]).any(1, keepdim=True)).float()
    pad = (lambda t: F.pad(t, (0, 0, 0, k - kk)) if t.dim() == 3 else F.pad(t, (0, k - kk))) if kk < k else (lambda t: t)   # K slots always
    return {"hm_target": hm, "anno_box_target": pad(anno), "ind_target": pad(ind), "mask_target": pad(ok.to(torch.uint8)), "segm_target": segm,
            "src_box_target": pad(src), "xsys_target": pad(xsys), "batch_gtboxes_src": gt.clone()}


# ---------------------------------------------------------------- losses ---------------------------------------------------------------
def gather_map(feat, ind):
    """center_utils._transpose_and_gather_feat (:250-259): (B, C, H, W), (B, K) -> (B, K, C)."""
    b, c = feat.shape[:2]
    return feat.view(b, c, -1).gather(2, ind.unsqueeze(1).expand(-1, c, -1)).transpose(1, 2)


def decode_rot_binres(reg, bins):
    """box_utils.decode_rot_binres (:366-406): (N, 2 bins) -> (N, 1) heading in (-pi, pi]."""
    per = 2 * math.pi / bins
    which = reg[:, :bins].argmax(1)
    res = reg[:, bins:].gather(1, which.unsqueeze(1)).squeeze(1) * (per / 2)
    ry = (which.float() * per + res) % (2 * math.pi)
    ry = torch.where(ry > math.pi, ry - 2 * math.pi, ry)
    return ry.view(-1, 1)


def center_losses(preds, tg, cfg, peaks=None):
    """CenterAFHeadTemplate.get_loss (center_af_head_template.py:193-460) on the seven head maps `preds` and the targets `tg`
    -> (total, dict of the eight weighted terms).  Tensor ops only; the one op of this repo it reaches is boxes_iou3d_gpu.
    `peaks` [B, K] (parity tests): heat-map cells to score in the IoU-score term instead of this run's own top K, so that two float
    implementations are compared on the same cells (two near-equal peaks may swap between them); the term records its cells in
    out["_iou_peaks"]."""
    w = cfg.loss_weights
    b = preds["hm"].shape[0]
    mask, ind = tg["mask_target"].bool(), tg["ind_target"]
    anno = tg["anno_box_target"]
    out = {}
    # heat map: CenterNetFocalLoss (loss_utils.py:410-462)
    p = torch.sigmoid(preds["hm"]).clamp(1e-4, 1 - 1e-4)
    t = tg["hm_target"]
    pos, neg = t.eq(1).float(), t.lt(1).float()
    pos_loss = (torch.log(p) * (1 - p).pow(2) * pos).sum()
    neg_loss = (torch.log(1 - p) * p.pow(2) * (1 - t).pow(4) * neg).sum()
    npos = pos.sum()
    out["hm"] = w["hm"] * torch.where(npos == 0, -neg_loss, -(pos_loss + neg_loss) / npos.clamp_min(1.0))
    # gathered L1 terms: CenterNetResLoss 'l1' (loss_utils.py:465-509): mean over the objects, sum over the channels
    any_obj = mask.any()

    def res(name, target):
        pred = gather_map(preds[name], ind)[mask]
        return F.l1_loss(pred, target[mask], reduction="none").mean(0).sum() if any_obj else pred.sum() * 0.0
    out["offset"] = w["offset"] * res("offset", anno[:, :, 0:2])
    out["height"] = w["height"] * res("height", anno[:, :, 2:3])
    out["dim"] = w["dim"] * res("dim", anno[:, :, 3:6])
    # heading: bin cross entropy + smooth-L1 of the normalised residual in the labelled bin (loss_utils.get_rot_binres_loss :334-404)
    bins = cfg.rot_bins
    rot_pred = gather_map(preds["rot"], ind)[mask]
    if any_obj:
        per = 2 * math.pi / bins
        heading = anno[:, :, 6][mask] % (2 * math.pi)
        shift = (heading + per / 2) % (2 * math.pi)
        bin_label = (shift / per).floor().long()
        res_label = (shift - (bin_label.float() * per + per / 2)) / (per / 2)
        onehot = F.one_hot(bin_label, bins).float()
        out["rot"] = w["rot"] * (F.cross_entropy(rot_pred[:, :bins], bin_label) +
                                 F.smooth_l1_loss((rot_pred[:, bins:] * onehot).sum(1), res_label))
    else:
        out["rot"] = rot_pred.sum() * 0.0
    # segmentation: sigmoid focal loss, every pixel weighted 1 / positives of its sample (:314-342)
    sp = preds["segm"].permute(0, 2, 3, 1).reshape(b, -1, 1)
    st = tg["segm_target"].permute(0, 2, 3, 1).reshape(b, -1, 1)
    weights = ((st == 0).float() + (st > 0).float()).squeeze(-1) / (st > 0).sum(1).float().clamp(min=1.0)
    out["segm"] = w["segm"] * sigmoid_focal(sp, st, weights).sum() / b
    # corner loss on the boxes decoded at the ground-truth centres (:344-365, 464-516; loss_utils.get_corner_loss_mse :246-281)
    k = ind.shape[1]
    off = gather_map(preds["offset"], ind)
    xs = (tg["xsys_target"][:, :, 0:1] + off[:, :, 0:1]) * cfg.feature_map_stride * cfg.voxel_size[0] + cfg.point_cloud_range[0]
    ys = (tg["xsys_target"][:, :, 1:2] + off[:, :, 1:2]) * cfg.feature_map_stride * cfg.voxel_size[1] + cfg.point_cloud_range[1]
    rot = decode_rot_binres(gather_map(preds["rot"], ind).reshape(b * k, -1), bins).view(b, k, 1)
    decoded = torch.cat((xs, ys, gather_map(preds["height"], ind), gather_map(preds["dim"], ind), rot), 2)
    if any_obj:
        pc, gc = box_corners(decoded[mask]), box_corners(tg["src_box_target"][mask])
        corner = sum(F.mse_loss(pc[:, :, a], gc[:, :, a]) for a in range(3))
    else:
        corner = decoded.sum() * 0.0
    out["corner"] = w["corner"] * corner / 3.0
    # IoU score: the K best peaks of the max-pooled heat map decoded to boxes, labelled by their best 3-D IoU with a box of the
    # predicted class (:367-460, 518-598; loss_utils.get_iouscore_loss_bce :284-331)
    with torch.no_grad():
        kq = cfg.num_iouscore_training_samples
        hm = preds["hm"].detach()
        heat = hm * (F.max_pool2d(hm, 3, stride=1, padding=1) == hm).float()                  # center_utils._nms
        nc, sy, sx = heat.shape[1:]
        top_s, top_i = torch.topk(heat.view(b, nc, -1), kq)                                     # center_utils._topk
        top_s2, top_j = torch.topk(top_s.view(b, -1), kq)
        inds = top_i.view(b, -1).gather(1, top_j) if peaks is None else peaks
        pxs, pys = (inds % sx).float().unsqueeze(-1), torch.div(inds, sx, rounding_mode="floor").float().unsqueeze(-1)
        offq = gather_map(preds["offset"].detach(), inds)
        bxs = (pxs + offq[:, :, 0:1]) * cfg.feature_map_stride * cfg.voxel_size[0] + cfg.point_cloud_range[0]
        bys = (pys + offq[:, :, 1:2]) * cfg.feature_map_stride * cfg.voxel_size[1] + cfg.point_cloud_range[1]
        rotq = decode_rot_binres(gather_map(preds["rot"].detach(), inds).reshape(b * kq, -1), bins).view(b, kq, 1)
        qboxes = torch.cat((bxs, bys, gather_map(preds["height"].detach(), inds), gather_map(preds["dim"].detach(), inds), rotq), 2)
        qcls = gather_map(heat, inds).argmax(-1) + 1                                             # (B, K) predicted class id
        gtb = tg["batch_gtboxes_src"]
        ious = []
        for i in range(b):     # per sample as the reference (boxes_iou3d_gpu is a pairwise op on one sample's boxes)
            valid = gtb[i, :, :7].sum(1) != 0
            g7, gl = gtb[i, valid, :7].contiguous(), gtb[i, valid, 7].long()
            best = qboxes.new_zeros(kq)
            if g7.shape[0] > 0:
                iou = iou3d_nms_utils.boxes_iou3d_gpu(qboxes[i].contiguous(), g7)               # (K, G)
                same = qcls[i][:, None] == gl[None, :]
                best = torch.where(same, iou, torch.zeros_like(iou)).amax(1)                   # get_max_iou_with_same_class
                best = torch.where(same.any(1), best, torch.zeros_like(best))
            ious.append(best)
        iou_gt = torch.stack(ious).view(-1)
        fg, bg = iou_gt > cfg.iou_fg_thresh, iou_gt < cfg.iou_bg_thresh
        label = torch.where(fg, torch.ones_like(iou_gt), torch.where(bg, torch.zeros_like(iou_gt),
                                                                      (iou_gt - cfg.iou_bg_thresh) / (cfg.iou_fg_thresh - cfg.iou_bg_thresh)))
    score = gather_map(preds["iouscore"], inds).reshape(-1)
    bce = F.binary_cross_entropy(torch.sigmoid(score), label, reduction="none")
    out["iouscore"] = w["iouscore"] * bce.sum() / max(bce.numel(), 1)
    total = sum(out.values())
    out["_iou_peaks"] = inds
    return total, out


# ---------------------------------------------------------------- test time -------------------------------------------------------------
_PEAK_MAPS = ("hm", "offset", "height", "dim", "rot", "iouscore")


def center_peaks_tensor_ops(preds, cfg, k, maxpool=True, cells=None):
    """predhm_based_predicted_boxes_generation_ssd (center_af_head_template.py:518-598; maxpool=False: ..._nomaxpooling, :600-667) as
    tensor ops, on the maps' device: the K best peaks of the max-pooled heat map of every sample, decoded.  -> dict: boxes (B, K, 7),
    cls (B, K, nc) the heat of every class at the cell, score (B, K) the raw IoU-score logit, cell (B, K) int64 = y * W + x,
    cls_id (B, K) int32.  This is the CPU route of `center_peaks` and the baseline its op is measured against.
    `cells` (B, K) int64: decode these cells instead of this call's own choice (cls_id is then the first maximal class there)."""
    hm = preds["hm"].detach()
    heat = hm * (F.max_pool2d(hm, 3, stride=1, padding=1) == hm).float() if maxpool else hm       # center_utils._nms
    b, nc, sy, sx = heat.shape
    if cells is None:
        top_s, top_i = torch.topk(heat.view(b, nc, -1), k)                                          # center_utils._topk
        top_s2, top_j = torch.topk(top_s.view(b, -1), k)
        inds = top_i.view(b, -1).gather(1, top_j)
        cls_id = torch.div(top_j, k, rounding_mode="floor").int()
    else:
        inds = cells
        cls_id = gather_map(heat, inds).argmax(-1).int()
    pxs, pys = (inds % sx).float().unsqueeze(-1), torch.div(inds, sx, rounding_mode="floor").float().unsqueeze(-1)
    offq = gather_map(preds["offset"].detach(), inds)
    bxs = (pxs + offq[:, :, 0:1]) * cfg.feature_map_stride * cfg.voxel_size[0] + cfg.point_cloud_range[0]
    bys = (pys + offq[:, :, 1:2]) * cfg.feature_map_stride * cfg.voxel_size[1] + cfg.point_cloud_range[1]
    rotq = decode_rot_binres(gather_map(preds["rot"].detach(), inds).reshape(b * k, -1), cfg.rot_bins).view(b, k, 1)
    boxes = torch.cat((bxs, bys, gather_map(preds["height"].detach(), inds), gather_map(preds["dim"].detach(), inds), rotq), 2)
    return {"boxes": boxes, "cls": gather_map(heat, inds).contiguous(), "score": gather_map(preds["iouscore"].detach(), inds).squeeze(-1),
            "cell": inds, "cls_id": cls_id}


def center_peaks(preds, cfg, k, maxpool=True):
    """The K best heat-map peaks of every sample, decoded (see center_peaks_tensor_ops for the result).  On a GPU: fv2p_center_peaks,
    two launches for the whole batch; anywhere else the tensor ops.  Order: descending heat, equal values by ascending
    class * H * W + cell - the reference's order wherever the K + 1 best values are distinct, the op's own definition where not."""
    hm = preds["hm"]
    if not hm.is_cuda:
        return center_peaks_tensor_ops(preds, cfg, k, maxpool)
    maps = [preds[n].detach() for n in _PEAK_MAPS]
    for n, t in zip(_PEAK_MAPS, maps):
        if t.dtype != torch.float32:
            raise TypeError(f"center_peaks: map '{n}' is {t.dtype}; the op takes float32 maps only")
    maps = [t.contiguous() for t in maps]
    b, nc, sy, sx = hm.shape
    boxes = torch.empty((b, k, 7), dtype=torch.float32, device=hm.device)
    cls = torch.empty((b, k, nc), dtype=torch.float32, device=hm.device)
    score = torch.empty((b, k), dtype=torch.float32, device=hm.device)
    cell = torch.empty((b, k), dtype=torch.int64, device=hm.device)
    cls_id = torch.empty((b, k), dtype=torch.int32, device=hm.device)
    with _nat.device_guard(hm.device):
        ws = _nat.workspace(int(_nat.lib().fv2p_center_peaks_ws_bytes(b, nc, sy, sx)), hm.device)
        _nat.call("fv2p_center_peaks", *maps, b, nc, sy, sx, int(k), int(bool(maxpool)), int(cfg.rot_bins), int(cfg.feature_map_stride),
                  float(cfg.voxel_size[0]), float(cfg.voxel_size[1]), float(cfg.point_cloud_range[0]), float(cfg.point_cloud_range[1]),
                  boxes, cls, score, cell, cls_id, ws, ws.numel(), _nat.stream())
    return {"boxes": boxes, "cls": cls, "score": score, "cell": cell, "cls_id": cls_id}


def _greedy_nms(boxes, thresh, post_max):
    """Rotated NMS of boxes (n, 7) already in descending score order -> the first post_max survivors' positions (int64, ascending).
    On a GPU the device pass of nms_gpu (one 4-byte copy for the count); on the host the greedy loop of iou3d_nms.cpp:121-135 on
    boxes_bev_iou_cpu."""
    if boxes.is_cuda:
        keep, cnt = iou3d_nms_cuda.nms_batch_device(boxes.unsqueeze(0).contiguous(), thresh, int(post_max), False)
        return keep[0, :int(cnt.item())]
    iou = iou3d_nms_utils.boxes_bev_iou_cpu(boxes.contiguous(), boxes.contiguous())
    alive, keep = torch.ones(boxes.shape[0], dtype=torch.bool), []
    for i in range(boxes.shape[0]):
        if alive[i]:
            keep.append(i)
            if len(keep) == post_max:
                break
            alive &= ~(iou[i] > thresh)
    return torch.tensor(keep, dtype=torch.int64)


def detections_tensor_ops(boxes, cls, loc_score, cfg, normalized=False):
    """The single-class-NMS branch of post_processing_withfgscores (detector3d_template.py:392-415) with
    class_agnostic_nms_withfgscore (model_nms_utils.py:27-50), sample by sample as the reference: mask, order (a stable descending
    sort: topk where the scores are distinct, ascending index where they repeat), NMS, index.  The result is padded to the layout of
    `detections`.  It is the CPU route and the baseline the op is measured against."""
    b, n = loc_score.shape
    post = min(cfg.nms_post_maxsize, n)
    out = {"boxes": boxes.new_zeros(b, post, 7), "scores": boxes.new_zeros(b, post), "labels": torch.zeros(b, post, dtype=torch.int32, device=boxes.device),
           "index": torch.full((b, post), -1, dtype=torch.int64, device=boxes.device), "count": torch.zeros(b, dtype=torch.int32, device=boxes.device)}
    for i in range(b):
        fg, label = torch.max(cls[i] if normalized else torch.sigmoid(cls[i]), dim=-1)
        original = (fg >= cfg.score_thresh).nonzero().view(-1)
        if original.numel() == 0:
            continue
        order = torch.sort(loc_score[i][original], descending=True, stable=True)[1][:cfg.nms_pre_maxsize]
        keep = _greedy_nms(boxes[i][original][order], cfg.nms_thresh, post)
        selected = original[order[keep]]
        m = selected.numel()
        out["boxes"][i, :m], out["scores"][i, :m] = boxes[i][selected], loc_score[i][selected]
        out["labels"][i, :m], out["index"][i, :m], out["count"][i] = (label[selected] + 1).int(), selected, m
    return out


def detections(boxes, cls, loc_score, cfg, normalized=False):
    """Detections of a batch of decoded candidates: boxes (B, N, 7), cls (B, N, nc) class scores (logits unless `normalized`),
    loc_score (B, N).  Candidates whose best class score reaches cfg.score_thresh, in descending loc_score (equal scores by ascending
    index), the first cfg.nms_pre_maxsize of them through rotated NMS at cfg.nms_thresh, the first cfg.nms_post_maxsize survivors.
    -> dict: boxes (B, P, 7), scores (B, P) the raw loc_score, labels (B, P) int32 from 1, index (B, P) int64 into the N candidates
    (-1 past the count), count (B) int32, P = min(nms_post_maxsize, N); rows past the count are zero.  On a GPU
    fv2p_detections_fgscore, with no host synchronisation; anywhere else detections_tensor_ops."""
    if not boxes.is_cuda:
        return detections_tensor_ops(boxes, cls, loc_score, cfg, normalized)
    for name, t in (("boxes", boxes), ("cls", cls), ("loc_score", loc_score)):
        if t.dtype != torch.float32:
            raise TypeError(f"detections: '{name}' is {t.dtype}; the op takes float32 only")
    boxes, cls, loc_score = boxes.detach().contiguous(), cls.detach().contiguous(), loc_score.detach().contiguous()
    b, n = loc_score.shape
    post, pre, dev = min(int(cfg.nms_post_maxsize), n), int(cfg.nms_pre_maxsize), boxes.device
    out = {"boxes": torch.empty((b, post, 7), dtype=torch.float32, device=dev), "scores": torch.empty((b, post), dtype=torch.float32, device=dev),
           "labels": torch.empty((b, post), dtype=torch.int32, device=dev), "index": torch.empty((b, post), dtype=torch.int64, device=dev),
           "count": torch.empty((b,), dtype=torch.int32, device=dev)}
    with _nat.device_guard(dev):
        ws = _nat.workspace(int(_nat.lib().fv2p_detections_fgscore_ws_bytes(b, n, pre, post)), dev)
        _nat.call("fv2p_detections_fgscore", boxes, cls, loc_score, b, n, cls.shape[-1], int(bool(normalized)), float(cfg.score_thresh),
                  float(cfg.nms_thresh), pre, post, out["boxes"], out["scores"], out["labels"], out["index"], out["count"], ws, ws.numel(),
                  _nat.stream())
    return out


class MGAFDetector(nn.Module):
    def __init__(self, cfg=MGAFConfig, offset_init_std=0.05):
        super().__init__()
        self.cfg = cfg
        self.backbone_3d = VoxelResBackBone8x(cfg.num_point_features, list(cfg.grid_size))     # BACKBONE_3D of both MGAF yamls
        self.backbone_2d = DCNBEVBackbone(cfg, 256)
        self.dense_head = CenterAFHead(cfg, self.backbone_2d.num_bev_features)
        self.taps = None    # set to a dict to collect head maps, targets and loss terms (parity tests)
        self.iou_peaks = None   # parity tests: the heat-map cells the IoU-score term scores ([B, K]; None = this run's own top K)
        # the reference zero-initialises the offset / mask predictors (all offsets 0 at step 0); a trained net has moved away from
        # that, so the replay starts them at small random values: sampling positions are fractional, as in any later step
        if offset_init_std > 0:
            for m in self.modules():
                if isinstance(m, (MdeformConvBlock, FeatureAdaption)):
                    nn.init.normal_(m.conv_offset_mask.weight, std=offset_init_std)

    def forward(self, voxel_features, voxel_coords, batch_size, gt_boxes=None):
        """-> the training loss of MGAF3DSSD.get_training_loss (detectors/mgaf_3dssd.py:24-34: the dense head's eight terms; the yaml has
        no point head).  Without gt_boxes: the surrogate of round 2 (mean square of every head map), a gradient through every layer."""
        out, _ = self.backbone_3d(voxel_features, voxel_coords, batch_size)
        dense = out.dense()
        spatial = dense.view(batch_size, dense.shape[1] * dense.shape[2], dense.shape[3], dense.shape[4])
        if getattr(self, "bev_channels_last", False):   # bench.py --bev-channels-last: the 2-D part in NHWC (the DCN kernels' layout)
            spatial = spatial.contiguous(memory_format=torch.channels_last)
        preds = self.dense_head(self.backbone_2d(spatial))
        if gt_boxes is None:
            return sum(p.square().mean() for p in preds.values())
        targets = center_targets(gt_boxes, self.cfg, dict(self.cfg.heads)["hm"])
        loss, terms = center_losses(preds, targets, self.cfg, peaks=self.iou_peaks)
        if self.taps is not None:
            self.taps.update(preds=preds, targets=targets, terms=terms)
        return loss

    def head_maps(self, voxel_features, voxel_coords, batch_size):
        """The seven head maps of a batch: sparse backbone, height compression, BEV backbone, centre head."""
        out, _ = self.backbone_3d(voxel_features, voxel_coords, batch_size)
        dense = out.dense()
        spatial = dense.view(batch_size, dense.shape[1] * dense.shape[2], dense.shape[3], dense.shape[4])
        if getattr(self, "bev_channels_last", False):
            spatial = spatial.contiguous(memory_format=torch.channels_last)
        return self.dense_head(self.backbone_2d(spatial))

    @torch.no_grad()
    def detect(self, preds):
        """Head maps -> the reference's pred_dicts: the eval branch of CenterAFHeadSingle.forward (center_af_head_single.py:130-138)
        and Detector3DTemplate.post_processing_withfgscores (detector3d_template.py:318-431, single-class NMS, no recall record).
        Two library calls and ONE device-to-host copy, of the per-sample counts."""
        peaks = center_peaks(preds, self.cfg, self.cfg.num_inference_samples)
        det = detections(peaks["boxes"], peaks["cls"], peaks["score"], self.cfg, normalized=False)   # cls_preds_normalized = False
        counts = det["count"].cpu().tolist()
        return [{"pred_boxes": det["boxes"][i, :c], "pred_scores": det["scores"][i, :c], "pred_labels": det["labels"][i, :c].long()}
                for i, c in enumerate(counts)]

    @torch.no_grad()
    def predict(self, voxel_features, voxel_coords, batch_size):
        """Test-time pass: a list of {'pred_boxes' (n, 7), 'pred_scores' (n,), 'pred_labels' (n,) from 1} per sample.  Normalisation
        layers follow the module's mode: call .eval() first to use their running statistics."""
        preds = self.head_maps(voxel_features, voxel_coords, batch_size)
        if self.taps is not None:
            self.taps.update(preds=preds)
        return self.detect(preds)
