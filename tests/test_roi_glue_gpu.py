"""The second-stage and point-head glue kernels (fv2p_roi_loss, fv2p_roipoint_pool3d_frame, fv2p_roi_grid, fv2p_point_loss) against the
tensor formulations they replace: IoUGuidedRoIHead.losses / reg_losses / canonical_targets / grid_points / pool_points and PointHead's
focal loss with KERNEL_GLUE off, never against the kernels themselves.

Gradients are held to autograd over the tensor form in float64 on the CPU.  Per case E = max |fp32 tensor form on the GPU - float64| is
measured first and the kernel may be off by 2 E + 1e-7 max|grad| (the factor 2: another summation order).  Where float64 is no yardstick
(saturated logits: float64 does not saturate there) the fp32 tensor form on the GPU is, with E = the spread between the fp32 GPU and fp32
CPU tensor results.  Every E and every kernel error is printed before it is asserted."""
import math
import os
import types

import numpy as np
import pytest
import torch

import fv2p_native as _nat
from fv2p_harness import fv2p_model as fm

from glue_util import hold, tensor_ops

pytestmark = pytest.mark.gpu
CFG = fm.FV2PConfig
PI = math.pi


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"pyref_{name}.npz"))


def roi_head():
    head = fm.IoUGuidedRoIHead.__new__(fm.IoUGuidedRoIHead)   # losses / grid_points read cfg only
    torch.nn.Module.__init__(head)
    head.cfg = CFG
    return head


def roi_loss_raw(rois, gt, iou, cls, reg8, canonical=False):
    """fv2p_roi_loss on CUDA tensors -> (loss5, dcls, dreg, canonical or None)."""
    r = cls.shape[0]
    out, dcls, dreg = cls.new_empty(5), torch.empty_like(cls), torch.empty_like(reg8)
    can = cls.new_empty(r, 7) if canonical else None
    _nat.call("fv2p_roi_loss", rois.reshape(-1, 7).contiguous(), gt.reshape(-1, gt.shape[-1]).contiguous(), iou.reshape(-1).contiguous(), cls.contiguous(),
              reg8.contiguous(), r, gt.shape[-1], float(CFG.cls_fg), float(CFG.cls_bg), CFG.cls_fg - CFG.cls_bg, float(CFG.reg_fg),
              (CFG.reg_fg - 0.5) * 2, 1.0 / 9.0, out, dcls, dreg, can, _nat.stream())
    return out, dcls, dreg, can


# ------------------------------------------------------------------------------------------------ second-stage loss: cases
def generic_case(r, seed, b=1):
    """float64 master arrays: rois (b, r/b, 7), their gt (b, r/b, 8), iou (b, r/b), cls (r, 1), reg8 (r, 8); every value float32-exact."""
    rng = np.random.default_rng(seed)
    n = r // b
    rois = np.concatenate((rng.uniform(-20, 20, (b, n, 3)), rng.uniform(1.0, 5.0, (b, n, 3)), rng.uniform(-PI, 3 * PI, (b, n, 1))), axis=2)
    gt = np.concatenate((rois[..., :3] + rng.normal(0, 0.3, (b, n, 3)), rois[..., 3:6] * np.exp(rng.normal(0, 0.1, (b, n, 3))),
                         rois[..., 6:7] + rng.normal(0, 0.4, (b, n, 1)) + PI * rng.integers(0, 2, (b, n, 1)), np.ones((b, n, 1))), axis=2)
    case = dict(rois=rois, gt=gt, iou=rng.uniform(0, 1, (b, n)), cls=rng.normal(0, 2, (r, 1)), reg8=rng.normal(0, 0.3, (r, 8)))
    return {k: v.astype(np.float32).astype(np.float64) for k, v in case.items()}


def case_no_fg():
    c = generic_case(64, 11)
    c["iou"] = c["iou"] * 0.5            # all below REG_FG_THRESH: both normalisers clamp to 1
    return c


def case_all_fg():
    c = generic_case(64, 12)
    c["iou"] = 0.76 + c["iou"] * 0.2
    return c


def case_thresholds():
    c = generic_case(8, 13)
    c["iou"][0, :3] = (0.25, 0.55, 0.75)   # CLS_BG, REG_FG and CLS_FG themselves (0.55 rounds to fp32 on the GPU: the same side of every threshold)
    return c


def heading_case(seed, d):
    c = generic_case(len(d), seed)
    c["rois"][0, :, 6] = np.linspace(-3.0, 3.0, len(d)).astype(np.float32)
    c["gt"][0, :, 6] = (c["rois"][0, :, 6] + np.array(d)).astype(np.float32)   # d = gt minus roi heading
    c["iou"][:] = 0.8
    return c


def case_headings():
    return heading_case(14, [0.3, 2.0, -2.0, -0.3, 1.2, 2.9, -1.2, -2.9, 4.0, 5.5, -4.0, -5.5])   # all four quadrants, either sign


def case_heading_boundaries():
    """+-pi/2, +-pi, 0 and 3 pi/2: the fold of the heading is decided by the last bit there, so float64 may fold the other way than fp32
    does (E then shows it); the kernel has to fold as the fp32 tensor form does, which the loss comparison holds it to."""
    return heading_case(18, [PI / 2, -PI / 2, PI, -PI, 0.0, 3 * PI / 2, -3 * PI / 2, 2 * PI])


def case_smooth_l1_edges():
    c = generic_case(8, 15)
    c["iou"][:] = 0.8
    c["gt"][0, 0, 2] = c["rois"][0, 0, 2]      # canonical z offset 0 -> target 0: the residual is the prediction itself
    c["reg8"][0, 3] = np.float32(1.0 / 9.0)    # exactly at beta: the linear branch (n < beta is strict)
    c["gt"][0, 1, 3] = c["rois"][0, 1, 3]      # log(1) = 0 target
    c["reg8"][1, 4] = 0.0                      # residual exactly 0: gradient 0
    return c


def case_zero_padded_gt():
    c = generic_case(8, 16)
    c["gt"][0, 2] = 0.0                        # a padding row sampled as a foreground target: sizes 0 meet the 1e-5 clamp
    c["iou"][0, 2] = 0.9
    return c


def case_saturated():
    c = generic_case(8, 17)
    c["cls"][:4, 0] = (30.0, -30.0, 120.0, -120.0)
    return c


LOSS_CASES = {
    "R1": lambda: generic_case(1, 1), "R3": lambda: generic_case(3, 2), "R257": lambda: generic_case(257, 3), "R384": lambda: generic_case(384, 4, b=3),
    "no_foreground": case_no_fg, "all_foreground": case_all_fg, "iou_thresholds": case_thresholds, "headings": case_headings,
    "heading_boundaries": case_heading_boundaries,
    "smooth_l1_edges": case_smooth_l1_edges, "zero_padded_gt": case_zero_padded_gt,
}


def tensor_form(case, device, dtype):
    """losses over canonical_targets in tensor ops -> (loss, d cls, d reg8) as float64 numpy."""
    t = {k: torch.tensor(v, dtype=dtype, device=device) for k, v in case.items()}
    cls, reg8 = t["cls"].requires_grad_(True), t["reg8"].requires_grad_(True)
    head = roi_head()
    with tensor_ops():
        loss = head.losses(t["rois"], t["gt"], head.canonical_targets(t["rois"], t["gt"]), t["iou"], cls, reg8[:, 1:], reg8[:, :1])
        dcls, dreg = torch.autograd.grad(loss, (cls, reg8))
    return float(loss), dcls.double().cpu().numpy(), dreg.double().cpu().numpy()


def kernel_form(case, device):
    t = {k: torch.tensor(v, dtype=torch.float32, device=device) for k, v in case.items()}
    cls, reg8 = t["cls"].requires_grad_(True), t["reg8"].requires_grad_(True)
    assert fm.KERNEL_GLUE
    loss = roi_head().losses(t["rois"], t["gt"], None, t["iou"], cls, reg8, None)
    dcls, dreg = torch.autograd.grad(loss, (cls, reg8))
    return float(loss), dcls.double().cpu().numpy(), dreg.double().cpu().numpy()


@pytest.mark.parametrize("name", sorted(LOSS_CASES))
def test_roi_loss_and_gradients_against_float64(gpu, name):
    """fv2p_roi_loss through IoUGuidedRoIHead.losses: the loss within 1e-5 of the tensor form, d cls and d reg within 2 E + 1e-7 max|grad| of float64."""
    case = LOSS_CASES[name]()
    l64, dcls64, dreg64 = tensor_form(case, "cpu", torch.float64)
    l32, dcls32, dreg32 = tensor_form(case, gpu, torch.float32)
    lk, dclsk, dregk = kernel_form(case, gpu)
    print(f"{name}: loss float64 {l64:.8f} fp32 tensor {l32:.8f} kernel {lk:.8f}")
    assert abs(lk - l32) < 1e-5 * max(1.0, abs(l32))
    assert name == "heading_boundaries" or abs(lk - l64) < 1e-5 * max(1.0, abs(l64))
    hold(name + " d cls", dclsk, dcls64, dcls32)
    hold(name + " d reg", dregk, dreg64, dreg32)
    if name == "heading_boundaries":
        # float64 folds some of these headings the other way, so E above is as large as the gradient itself and that bound holds nothing:
        # here the fp32 tensor form on the GPU is the yardstick as well, E = its spread to the fp32 tensor form on the CPU
        _, dclsc, dregc = tensor_form(case, "cpu", torch.float32)
        hold(name + " d cls (fp32 yardstick)", dclsk, dcls32, dclsc)
        hold(name + " d reg (fp32 yardstick)", dregk, dreg32, dregc)
    if name == "no_foreground":
        assert (dregk == 0).all(), "no roi above REG_FG_THRESH: the reg, corner and IoU gradients are exactly 0"


def test_roi_loss_saturated_logits_against_the_fp32_tensor_form(gpu):
    """Logits of +-30 and +-120: F.binary_cross_entropy's backward divides by max(p (1 - p), 1e-12) and the sigmoid's multiplies by
    p (1 - p), so the gradient is 0 once the sigmoid saturates in fp32 (float64 does not saturate there: no yardstick).  Against the fp32
    tensor form on the GPU, E = its spread to the fp32 tensor form on the CPU."""
    case = case_saturated()
    lg, dclsg, dregg = tensor_form(case, gpu, torch.float32)
    lc, dclsc, dregc = tensor_form(case, "cpu", torch.float32)
    lk, dclsk, dregk = kernel_form(case, gpu)
    print(f"saturated: loss fp32 gpu {lg:.8f} fp32 cpu {lc:.8f} kernel {lk:.8f}; d cls kernel {dclsk[:4, 0]} tensor {dclsg[:4, 0]}")
    assert abs(lk - lg) < 1e-5 * max(1.0, abs(lg))
    hold("saturated d cls", dclsk, dclsg, dclsc)
    hold("saturated d reg", dregk, dregg, dregc)
    assert dclsk[0, 0] == 0 and dclsk[2, 0] == 0 and dclsk[3, 0] == 0   # sigmoid(30) == 1, sigmoid(+-120) in {1, 0} in fp32


def test_roi_loss_twice_gives_the_same_bits(gpu):
    case = generic_case(384, 5, b=3)
    t = {k: torch.tensor(v, dtype=torch.float32, device=gpu) for k, v in case.items()}
    a = roi_loss_raw(t["rois"], t["gt"], t["iou"], t["cls"], t["reg8"])
    b = roi_loss_raw(t["rois"], t["gt"], t["iou"], t["cls"], t["reg8"])
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


def test_roi_loss_on_the_reference_fixtures(gpu, golden_dir):
    """pyref_roi_losses (total, class and IoU parts), pyref_roi_reg_loss (regression and corner parts, its mask as IoUs on either side of
    the threshold) and pyref_canonical_targets (the kernel's canonical boxes), each within 1e-5 (relative, floor 1)."""
    close = lambda a, b: abs(float(a) - float(b)) < 1e-5 * max(1.0, abs(float(b)))
    g = load(golden_dir, "roi_losses")
    t = lambda k: torch.from_numpy(g[k]).to(gpu)
    reg8 = torch.cat((t("rcnn_iou"), t("rcnn_reg")), dim=1)
    out, _, _, can = roi_loss_raw(t("rois"), t("gt_src"), t("ious"), t("rcnn_cls"), reg8, canonical=True)
    out = out.cpu().numpy()
    print("roi_losses fixture: kernel", out, "reference total", float(g["total"]), "cls", float(g["loss_cls"]), "iou", float(g["loss_iou"]), "reg", float(g["loss_reg"]))
    assert close(out[0], g["total"]) and close(out[1], g["loss_cls"]) and close(out[4], g["loss_iou"]) and close(out[2] + out[3], g["loss_reg"])
    want = g["gt_canonical"].reshape(-1, 8)[:, :7]
    assert np.abs(can.cpu().numpy() - want).max() < 1e-5 * max(1.0, np.abs(want).max())
    total = roi_head().losses(t("rois"), t("gt_src"), None, t("ious"), t("rcnn_cls"), t("rcnn_reg"), t("rcnn_iou"))   # the route with the row in two pieces
    assert close(total.item(), g["total"])

    g = load(golden_dir, "roi_reg_loss")
    iou = torch.from_numpy(np.where(g["valid"] > 0, 0.9, 0.1).astype(np.float32)).to(gpu)
    reg8 = torch.cat((torch.zeros(g["rcnn_reg"].shape[0], 1), torch.from_numpy(g["rcnn_reg"])), dim=1).to(gpu)
    out = roi_loss_raw(t("rois"), t("gt_src"), iou, torch.zeros(reg8.shape[0], 1, device=gpu), reg8)[0].cpu().numpy()
    print("roi_reg_loss fixture: kernel reg", out[2], "corner", out[3], "reference", float(g["loss_reg"]), float(g["loss_corner"]))
    assert close(out[2], g["loss_reg"]) and close(out[3], g["loss_corner"])

    g = load(golden_dir, "canonical_targets")
    r = g["rois"].shape[0] * g["rois"].shape[1]
    z = torch.zeros(r, 8, device=gpu)
    can = roi_loss_raw(t("rois"), t("gt_of_rois"), z[:, 0].contiguous(), z[:, :1].contiguous(), z, canonical=True)[3].cpu().numpy()
    want = g["canonical"].reshape(-1, 8)[:, :7]
    print("canonical_targets fixture: max |kernel - reference|", np.abs(can - want).max())
    assert np.abs(can - want).max() < 1e-5 * max(1.0, np.abs(want).max())


# ------------------------------------------------------------------------------------------------ grid geometry
def test_roi_grid_against_grid_points_and_the_fixture(gpu, golden_dir):
    g = load(golden_dir, "roi_grid_points")
    head = roi_head()
    rois = torch.from_numpy(g["rois"]).to(gpu)
    n = CFG.grid_size_roi
    local, column, corners = fm.roi_grid_geometry(rois, n)
    again = fm.roi_grid_geometry(rois, n)
    assert all(torch.equal(a, b) for a, b in zip((local, column, corners), again))
    with tensor_ops():
        world_t, local_t = head.grid_points(rois)
    col_t = world_t.view(-1, n * n, n, 3)[:, :, 0]
    corners_t = rois.reshape(-1, 7)[:, None, 3:6] * (fm.dconst(rois, fm._CORNER_SIGNS, rois.dtype) / 2)[None]
    err = lambda a, b: float((a - b).abs().max())
    print("roi_grid: local", err(local, local_t), "column", err(column, col_t), "corners", err(corners, corners_t))
    assert local.shape == local_t.shape and column.shape == col_t.shape and corners.shape == corners_t.shape
    assert err(local, local_t) < 1e-5 and err(column, col_t) < 1e-5 and err(corners, corners_t) < 1e-5
    assert np.abs(local.cpu().numpy() - g["local"]).max() < 1e-5
    assert np.abs(column.cpu().numpy() - g["world"].reshape(-1, n * n, n, 3)[:, :, 0]).max() < 1e-5 * max(1.0, np.abs(g["world"]).max())


# ------------------------------------------------------------------------------------------------ pooled points in the roi's frame
def pool_head(sampled, extra):
    from pcdet.ops.roipoint_pool3d import roipoint_pool3d_utils
    return types.SimpleNamespace(cfg=types.SimpleNamespace(depth_normalizer=70.0),
                                 roipoint_pool3d_layer=roipoint_pool3d_utils.RoIPointPool3d(num_sampled_points=sampled, pool_extra_width=list(extra)))


def test_pool_in_frame_on_the_reference_fixture(gpu, golden_dir):
    g = load(golden_dir, "roi_point_pool")
    t = lambda k: torch.from_numpy(g[k]).to(gpu)
    pooled = fm.IoUGuidedRoIHead.pool_points(pool_head(64, (0.4, 0.4, 0.4)), t("keypoints"), t("point_features"), t("point_scores"), t("rois")).cpu().numpy()
    want = g["pooled"]
    assert pooled.shape == want.shape
    assert np.array_equal(pooled[..., 3], want[..., 3]) and np.array_equal(pooled[..., 5:], want[..., 5:]), "pooled point order / [score, features] payload differs"
    print("pool fixture: depth", np.abs(pooled[..., 4] - want[..., 4]).max(), "coordinates", np.abs(pooled[..., :3] - want[..., :3]).max())
    assert np.abs(pooled[..., 4] - want[..., 4]).max() < 1e-5 and np.abs(pooled[..., :3] - want[..., :3]).max() < 1e-5
    empty = np.abs(want).reshape(want.shape[0], -1).sum(1) == 0
    assert empty.sum() == 4 and (pooled[empty] == 0).all()


def test_pool_in_frame_against_the_tensor_route(gpu):
    """B = 2 with 700 points (no multiple of the 1024-thread workgroup), C = 128 (rows of 133 floats), S = 512; per sample one empty box, one
    with fewer than S inside points (wrap-around), one with more than S, one rotated by 2.5 rad.  Which point landed in which slot exactly
    (feature 0 carries the point's index), coordinates and depth within 1e-5."""
    rng = np.random.default_rng(21)
    b, n, c, s = 2, 700, 128, 512
    key = rng.uniform(-4, 4, (b, n, 3)).astype(np.float32) + np.array([20.0, 0.0, 0.0], dtype=np.float32)
    feats = rng.normal(0, 1, (b * n, c)).astype(np.float32)
    feats[:, 0] = np.arange(b * n)
    scores = rng.uniform(0, 1, b * n).astype(np.float32)
    rois = np.array([[[60.0, 30.0, 0.0, 2.0, 2.0, 2.0, 0.3],       # empty
                      [20.0, 0.0, 0.0, 2.0, 2.0, 2.0, 0.4],        # a few dozen points: wrap-around
                      [20.0, 0.0, 0.0, 9.0, 9.0, 9.0, -0.7],       # everything: more than S
                      [21.0, 1.0, 0.5, 4.0, 1.5, 3.0, 2.5]]] * b, dtype=np.float32)
    rois[1, :, 0] += 0.25
    t = lambda a: torch.from_numpy(a).to(gpu)
    head = pool_head(s, (1.0, 1.0, 1.0))
    got = fm.IoUGuidedRoIHead.pool_points(head, t(key), t(feats), t(scores), t(rois))
    again = fm.IoUGuidedRoIHead.pool_points(head, t(key), t(feats), t(scores), t(rois))
    with tensor_ops():
        want = fm.IoUGuidedRoIHead.pool_points(head, t(key), t(feats), t(scores), t(rois))
    assert torch.equal(got, again) and got.shape == want.shape == (b * 4, s, 5 + c)
    got, want = got.cpu().numpy(), want.cpu().numpy()
    inside = [len(np.unique(want[i, :, 5])) for i in range(b * 4)]
    print("pool: distinct points per box", inside, "coordinates", np.abs(got[..., :3] - want[..., :3]).max(), "depth", np.abs(got[..., 4] - want[..., 4]).max())
    assert (want[0] == 0).all() and 1 < inside[1] < s and inside[2] == s and 1 < inside[3] < s
    assert np.array_equal(got[..., 5], want[..., 5]), "another point in some slot"
    assert np.array_equal(got[..., 3], want[..., 3]) and np.array_equal(got[..., 5:], want[..., 5:])
    assert np.abs(got[..., :3] - want[..., :3]).max() < 1e-5 and np.abs(got[..., 4] - want[..., 4]).max() < 1e-5
    assert (got[0] == 0).all() and (got[4] == 0).all()


# ------------------------------------------------------------------------------------------------ point-head loss
def point_case(n, kind, seed):
    rng = np.random.default_rng(seed)
    logits = rng.normal(0, 2, (n, 1)).astype(np.float32)
    labels = {"mixed": rng.integers(-1, 2, n), "zero_logits": rng.integers(-1, 2, n), "no_positives": rng.integers(-1, 1, n),
              "all_ignored": np.full(n, -1)}[kind].astype(np.int64)
    if kind == "zero_logits":   # a logit of exactly 0 on a positive, a negative and an ignored point: autograd's clamp(min=0) and sgn(0) = 0 there
        logits[:3, 0], labels[:3] = 0.0, (1, 0, -1)
    return logits, labels


def point_tensor_form(logits, labels, device, dtype):
    x = torch.tensor(logits, dtype=dtype, device=device).requires_grad_(True)
    lab = torch.from_numpy(labels).to(device)
    pos = lab > 0
    w = ((lab == 0) | pos).to(dtype) / pos.sum().to(dtype).clamp_min(1.0)
    loss = fm.sigmoid_focal(x, pos.to(dtype).unsqueeze(-1), w).sum() * CFG.point_cls_weight
    grad, = torch.autograd.grad(loss, x)
    return float(loss), grad.double().cpu().numpy(), torch.sigmoid(x.detach()).view(-1).double().cpu().numpy()


@pytest.mark.parametrize("n,kind", [(1, "mixed"), (63, "mixed"), (65, "mixed"), (1000, "mixed"), (65, "no_positives"), (63, "all_ignored"), (1000, "no_positives"),
                                    (65, "zero_logits")])
def test_point_loss_against_float64(gpu, n, kind):
    logits, labels = point_case(n, kind, 100 + n)
    l64, g64, s64 = point_tensor_form(logits, labels, "cpu", torch.float64)
    l32, g32, _ = point_tensor_form(logits, labels, gpu, torch.float32)
    x = torch.from_numpy(logits).to(gpu).requires_grad_(True)
    lab = torch.from_numpy(labels).to(gpu)
    loss, score = fm.PointLossFn.apply(x, lab, CFG.point_cls_weight)
    grad, = torch.autograd.grad(loss, x)
    loss2, score2 = fm.PointLossFn.apply(x, lab, CFG.point_cls_weight)
    grad2, = torch.autograd.grad(loss2, x)
    assert torch.equal(loss, loss2) and torch.equal(score, score2) and torch.equal(grad, grad2)
    print(f"point loss n {n} {kind}: float64 {l64:.8f} fp32 tensor {l32:.8f} kernel {float(loss):.8f}")
    assert abs(float(loss) - l64) < 1e-5 * max(1.0, abs(l64))
    hold(f"point loss n {n} {kind} d logits", grad.double().cpu().numpy(), g64, g32)
    assert np.abs(score.double().cpu().numpy() - s64).max() < 1e-6 and not score.requires_grad
    if kind == "all_ignored":
        assert float(loss) == 0 and (grad == 0).all()


def test_point_loss_on_the_reference_fixture(gpu, golden_dir):
    g = load(golden_dir, "point_head")
    loss, score = fm.PointLossFn.apply(torch.from_numpy(g["logits"]).to(gpu), torch.from_numpy(g["labels"]).to(gpu), CFG.point_cls_weight)
    print("point_head fixture: kernel", float(loss), "reference", float(g["loss"]))
    assert abs(float(loss) - float(g["loss"])) < 1e-5 * max(1.0, abs(float(g["loss"])))
    assert score.shape == (g["logits"].shape[0],)
