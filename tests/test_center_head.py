"""Centre head at test time: heat-map peak decode (fv2p_center_peaks) and detections (fv2p_detections_fgscore), and
MGAFDetector.predict on top of them.

What each op is held to:
  selection   a numpy restatement of the rule written here without project code: heat = hm * (hm == 3x3 maximum), the K first
              entries of a STABLE sort on (-value, class * H * W + cell).  Cells and class ids must be equal to it.  On the
              reference-written fixture (tests/golden/pyref_center_losses.npz) the rule gives the cells of the reference's two-stage
              topk, and the decoded boxes are the reference's `decoded_topk_boxes` bit for bit.
  decode      center_peaks_tensor_ops (the tensor-op restatement of center_af_head_template.py:518-598) on the same device at the same
              cells, bit for bit; a heading within 1e-3 of +-pi is compared modulo 2 pi (the fold `> pi` may fall either way there).
  detections  the per-sample composition mask -> topk -> nms_gpu(NMS_POST_MAXSIZE) -> index of model_nms_utils.py:27-50, written here:
              indices and counts equal, boxes and scores are copies and bit-equal."""
import math
import os

import numpy as np
import pytest
import torch

import fv2p_native as _nat
from fv2p_harness import mgaf_model as mm
from pcdet.ops.iou3d_nms import iou3d_nms_utils

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PEAK_MAPS = ("hm", "offset", "height", "dim", "rot", "iouscore")


# ------------------------------------------------------------------ the rule, in numpy ------------------------------------------------
def np_heat(hm, maxpool=True):
    if not maxpool:
        return hm.copy()
    b, c, h, w = hm.shape
    pad = np.full((b, c, h + 2, w + 2), -np.inf, np.float32)
    pad[:, :, 1:-1, 1:-1] = hm
    m = np.full_like(hm, -np.inf)
    for dy in range(3):
        for dx in range(3):
            m = np.maximum(m, pad[:, :, dy:dy + h, dx:dx + w])
    return hm * (hm == m).astype(np.float32)


def np_select(heat, k):
    """-> (cell [B, k], cls_id [B, k], flat index [B, k]): descending value, ties by ascending class * H * W + cell."""
    b, c, h, w = heat.shape
    flat = np.stack([np.argsort(-heat[i].reshape(-1), kind="stable")[:k] for i in range(b)])
    return flat % (h * w), flat // (h * w), flat


def best_are_distinct(heat, k):
    """the k + 1 best values of every sample are distinct: there the reference's topk and the rule agree"""
    for i in range(heat.shape[0]):
        top = np.sort(heat[i].reshape(-1))[::-1][:k + 1]
        if top.size > 1 and np.min(top[:-1] - top[1:]) <= 0:
            return False
    return True


def fixture():
    fix = np.load(os.path.join(GOLD, "pyref_center_losses.npz"))
    cfg = type("Cfg", (mm.MGAFConfig,), {"point_cloud_range": tuple(float(v) for v in fix["point_cloud_range"]),
                                         "voxel_size": tuple(float(v) for v in fix["voxel_size"])})
    return fix, cfg, {n: torch.from_numpy(fix["pred_" + n]) for n in PEAK_MAPS}


def random_maps(b, nc, h, w, bins, seed):
    g = torch.Generator().manual_seed(seed)
    chans = {"hm": nc, "offset": 2, "height": 1, "dim": 3, "rot": 2 * bins, "iouscore": 1}
    return {n: torch.randn(b, c, h, w, generator=g) for n, c in chans.items()}


def cfg_with(**kw):
    return type("Cfg", (mm.MGAFConfig,), kw)


# ------------------------------------------------------------------ CPU tests ----------------------------------------------------------
def test_tensor_op_peaks_equal_the_reference_boxes_bit_for_bit():
    fix, cfg, preds = fixture()
    got = mm.center_peaks(preds, cfg, 24)            # a CPU map: the tensor-op route
    diff = np.abs(got["boxes"].numpy() - fix["decoded_topk_boxes"]).reshape(-1, 7).max(0)
    print("max abs difference per box column:", diff)
    assert np.array_equal(got["boxes"].numpy().view(np.int32), fix["decoded_topk_boxes"].view(np.int32))
    assert got["cls"].shape == (3, 24, 3) and got["score"].shape == (3, 24) and got["cell"].dtype == torch.int64 and got["cls_id"].dtype == torch.int32


@pytest.mark.parametrize("k", [24, 50])
def test_selection_rule_gives_the_two_stage_topk_on_the_fixture(k):
    fix, cfg, preds = fixture()
    heat = np_heat(fix["pred_hm"])
    assert best_are_distinct(heat, k)
    cell, cls_id, _ = np_select(heat, k)
    got = mm.center_peaks_tensor_ops(preds, cfg, k)
    assert np.array_equal(got["cell"].numpy(), cell)
    assert np.array_equal(got["cls_id"].numpy(), cls_id)
    positive = (heat.reshape(3, -1) > 0).sum(1)
    assert positive.min() > k, positive


def test_workspace_queries_are_pure_host_functions():
    lib = _nat.lib()
    peaks, det = lib.fv2p_center_peaks_ws_bytes, lib.fv2p_detections_fgscore_ws_bytes
    assert peaks(1, 1, 1, 1) > 0 and peaks(4, 3, 200, 176) >= 4 * 3 * 200 * 176 * 4
    assert det(1, 1, 1, 1) > 0 and det(4, 50, 4096, 50) > 0
    for b in range(1, 9):
        assert peaks(b + 1, 3, 40, 35) >= peaks(b, 3, 40, 35)
        assert det(b + 1, 300, 4096, 100) >= det(b, 300, 4096, 100)
    for bad in ((0, 3, 40, 35), (2, 0, 40, 35), (2, 3, -1, 35), (2, 3, 40, 0)):
        assert peaks(*bad) == 0
    for bad in ((0, 50, 10, 10), (2, 0, 10, 10), (2, 50, 0, 10), (2, 50, 10, -3)):
        assert det(*bad) == 0


def scene(n, seed, cluster=0.5, spacing=8.0):
    """n boxes: car-sized, on a grid `spacing` apart, a share `cluster` of them moved onto an earlier box (a few centimetres off)."""
    g = torch.Generator().manual_seed(seed)
    side = int(math.ceil(math.sqrt(n)))
    idx = torch.arange(n)
    boxes = torch.zeros(n, 7)
    boxes[:, 0] = (idx % side).float() * spacing + torch.rand(n, generator=g)
    boxes[:, 1] = torch.div(idx, side, rounding_mode="floor").float() * spacing - 20 + torch.rand(n, generator=g)
    boxes[:, 2] = -1 + 0.2 * torch.rand(n, generator=g)
    boxes[:, 3:6] = torch.tensor([3.9, 1.6, 1.5]) + 0.3 * torch.rand(n, 3, generator=g)
    boxes[:, 6] = (torch.rand(n, generator=g) * 2 - 1) * math.pi
    for i in range(1, n):
        if torch.rand(1, generator=g).item() < cluster:
            j = int(torch.randint(0, i, (1,), generator=g))
            boxes[i] = boxes[j] + 0.03 * torch.randn(7, generator=g)
    return boxes


def host_nms(boxes, thresh):
    """the greedy loop of iou3d_nms.cpp:121-135 on boxes_bev_iou_cpu"""
    iou = iou3d_nms_utils.boxes_bev_iou_cpu(boxes.contiguous(), boxes.contiguous())
    keep, dead = [], torch.zeros(boxes.shape[0], dtype=torch.bool)
    for i in range(boxes.shape[0]):
        if not dead[i]:
            keep.append(i)
            dead |= iou[i] > thresh
    return torch.tensor(keep, dtype=torch.int64, device=boxes.device)


def device_nms(boxes, thresh, post):
    """nms_gpu on boxes already in their order: strictly falling stand-in scores keep its own sort from reordering equal ones"""
    falling = torch.arange(boxes.shape[0], 0, -1, device=boxes.device, dtype=torch.float32)
    return iou3d_nms_utils.nms_gpu(boxes, falling, thresh, NMS_POST_MAXSIZE=post)[0]


def literal_detections(boxes, cls, loc, cfg, normalized, stable=False):
    """post_processing_withfgscores :392-415 + class_agnostic_nms_withfgscore, one sample: -> (selected, scores, labels, boxes)"""
    cls_preds = cls if normalized else torch.sigmoid(cls)
    cls_preds, label_preds = torch.max(cls_preds, dim=-1)
    label_preds = label_preds + 1
    scores_mask = cls_preds >= cfg.score_thresh
    box_scores, box_preds = loc[scores_mask], boxes[scores_mask]
    selected = torch.zeros(0, dtype=torch.int64, device=boxes.device)
    if box_scores.shape[0] > 0:
        kk = min(cfg.nms_pre_maxsize, box_scores.shape[0])
        if stable:    # equal scores: torch.topk promises no order, the op's rule is ascending index
            box_scores_nms, indices = (t[:kk] for t in torch.sort(box_scores, descending=True, stable=True))
        else:
            box_scores_nms, indices = torch.topk(box_scores, k=kk)
        boxes_for_nms = box_preds[indices]
        if boxes.is_cuda:
            keep_idx = device_nms(boxes_for_nms[:, 0:7], cfg.nms_thresh, cfg.nms_post_maxsize)
        else:
            keep_idx = host_nms(boxes_for_nms[:, 0:7], cfg.nms_thresh)
        selected = indices[keep_idx[:cfg.nms_post_maxsize]]
    original_idxs = scores_mask.nonzero().view(-1)
    selected = original_idxs[selected]
    return selected, loc[selected], label_preds[selected], boxes[selected]


def check_detections(boxes, cls, loc, cfg, normalized, stable=False, exact_threshold=False):
    """`mm.detections` on the tensors' device against the literal composition, sample by sample; -> the counts"""
    thr = float(np.float32(cfg.score_thresh))
    fg64 = (cls.double() if normalized else torch.sigmoid(cls.double())).amax(-1).cpu()
    near = (fg64 - thr).abs() <= 1e-6
    if exact_threshold:   # scores that ARE the threshold pin `>=`; everything else stays clear of it
        near &= fg64 != thr
    assert not near.any(), "a foreground score within 1e-6 of the threshold"
    if not stable:
        for s in loc.cpu():
            assert s.unique().numel() == s.numel(), "loc scores repeat"
    got = mm.detections(boxes, cls, loc, cfg, normalized=normalized)
    b, n = loc.shape
    post = min(cfg.nms_post_maxsize, n)
    assert got["boxes"].shape == (b, post, 7) and got["index"].dtype == torch.int64 and got["count"].dtype == torch.int32 and got["labels"].dtype == torch.int32
    counts = got["count"].cpu().tolist()
    for i in range(b):
        sel, scores, labels, bx = literal_detections(boxes[i], cls[i], loc[i], cfg, normalized, stable)
        c = counts[i]
        assert c == sel.numel(), (i, c, sel.numel())
        assert torch.equal(got["index"][i, :c], sel), i
        assert torch.equal(got["boxes"][i, :c].view(torch.int32), bx.view(torch.int32))
        assert torch.equal(got["scores"][i, :c].view(torch.int32), scores.view(torch.int32))
        assert torch.equal(got["labels"][i, :c].long(), labels)
        assert (got["index"][i, c:] == -1).all() and (got["boxes"][i, c:] == 0).all() and (got["scores"][i, c:] == 0).all() and (got["labels"][i, c:] == 0).all()
    return counts


def detection_case(name, dev="cpu"):
    """-> (boxes, cls, loc, cfg, normalized, flags of check_detections, expected property of the counts)"""
    g = torch.Generator().manual_seed(7)
    base = dict(score_thresh=0.501, nms_thresh=0.1, nms_pre_maxsize=4096, nms_post_maxsize=500)

    def batch(b, n, cluster=0.5, nc=3):
        boxes = torch.stack([scene(n, 10 + i, cluster) for i in range(b)])
        cls = torch.randn(b, n, nc, generator=g) * 2
        loc = torch.randn(b, n, generator=g)
        return boxes, cls, loc
    flags, normalized, want = {}, False, lambda c: True
    if name == "nothing_passes":
        boxes, cls, loc = batch(2, 40)
        cls = -cls.abs() - 1.0
        want = lambda c: c == [0, 0]
    elif name == "everything_passes":
        boxes, cls, loc = batch(2, 40, cluster=0.0)
        cls = cls.abs() + 1.0
        want = lambda c: c == [40, 40]
    elif name == "normalized_at_the_threshold":
        boxes, cls, loc = batch(2, 40, cluster=0.0)
        cls = torch.rand(2, 40, 3, generator=g) * 0.45                    # all below the threshold ...
        cls[:, 0::3, 1] = float(np.float32(0.501))                        # ... but every third exactly on it: it passes (>=)
        normalized, flags = True, {"exact_threshold": True}
        want = lambda c: c == [14, 14]
    elif name == "one_candidate":
        boxes, cls, loc = batch(3, 1)
        cls[0], cls[1], cls[2] = 2.0, -2.0, 1.0
        want = lambda c: c == [1, 0, 1]
    elif name == "cluster":
        boxes, cls, loc = batch(2, 200, cluster=0.9)
        cls = cls.abs() + 0.5
        want = lambda c: all(0 < v < 100 for v in c)
    elif name == "post_max_cuts":
        boxes, cls, loc = batch(2, 70, cluster=0.0)
        cls = cls.abs() + 0.5
        base["nms_post_maxsize"] = 5
        want = lambda c: c == [5, 5]
    elif name == "pre_max_cuts":
        boxes, cls, loc = batch(2, 70, cluster=0.0)
        cls = cls.abs() + 0.5
        base["nms_pre_maxsize"] = 10
        want = lambda c: c == [10, 10]
    elif name == "counts_differ":
        boxes, cls, loc = batch(3, 130, cluster=0.4)
        cls[0] = -cls[0].abs() - 1.0
        cls[1] = cls[1].abs() + 1.0
        cls[2, 0::2] = -cls[2, 0::2].abs() - 1.0
        want = lambda c: c[0] == 0 and c[1] > c[2] > 0
    elif name == "equal_loc_scores":
        boxes, cls, loc = batch(2, 90, cluster=0.5)
        loc = torch.round(loc * 2) / 2                                     # a handful of distinct values, -0.0 and 0.0 among them
        loc[0, 5] = -0.0
        flags = {"stable": True}
        want = lambda c: all(v > 0 for v in c)
    else:
        raise KeyError(name)
    return boxes.to(dev), cls.to(dev), loc.to(dev), cfg_with(**base), normalized, flags, want


DETECTION_CASES = ["nothing_passes", "everything_passes", "normalized_at_the_threshold", "one_candidate", "cluster", "post_max_cuts",
                   "pre_max_cuts", "counts_differ", "equal_loc_scores"]


@pytest.mark.parametrize("name", ["nothing_passes", "normalized_at_the_threshold", "one_candidate", "cluster", "post_max_cuts", "pre_max_cuts",
                                  "equal_loc_scores"])
def test_detections_on_the_host_equal_the_literal_composition(name):
    boxes, cls, loc, cfg, normalized, flags, want = detection_case(name)
    boxes, cls, loc = boxes[:, :24], cls[:, :24], loc[:, :24]              # a handful of boxes: the host IoU is a Python-speed loop
    check_detections(boxes, cls, loc, cfg, normalized, **flags)


# ------------------------------------------------------------------ GPU tests: center_peaks --------------------------------------------
def check_peaks(preds, cfg, k, maxpool, dev):
    """the op on `dev` against the numpy rule (cells, class ids) and the tensor ops at the same cells (everything else); -> the op's result"""
    heat = np_heat(preds["hm"].numpy(), maxpool)
    cell, cls_id, _ = np_select(heat, k)
    on_dev = {n: t.to(dev) for n, t in preds.items()}
    got = mm.center_peaks(on_dev, cfg, k, maxpool=maxpool)
    assert got["cell"].dtype == torch.int64 and got["cls_id"].dtype == torch.int32
    assert np.array_equal(got["cell"].cpu().numpy(), cell)
    assert np.array_equal(got["cls_id"].cpu().numpy(), cls_id)
    ref = mm.center_peaks_tensor_ops(on_dev, cfg, k, maxpool=maxpool, cells=got["cell"])
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(got["boxes"][..., :6]), bits(ref["boxes"][..., :6]))
    assert torch.equal(bits(got["cls"]), bits(ref["cls"]))          # bit for bit: the -0.0 of a suppressed negative logit included
    assert torch.equal(bits(got["score"]), bits(ref["score"]))
    a, r = got["boxes"][..., 6], ref["boxes"][..., 6]
    edge = (r.abs() - math.pi).abs() < 1e-3
    assert torch.equal(bits(a[~edge]), bits(r[~edge]))
    turn = torch.remainder(a[edge] - r[edge] + math.pi, 2 * math.pi) - math.pi
    assert (turn.abs() <= 1e-6).all()
    assert (a > -math.pi - 1e-6).all() and (a <= math.pi).all()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("k", [24, 50])
@pytest.mark.parametrize("maxpool", [True, False])
def test_peaks_of_the_reference_fixture(gpu, k, maxpool):
    """(a), (h): 3 x 3 x 40 x 35, rows of 35 floats: the scalar-access form of the key kernel"""
    fix, cfg, preds = fixture()
    got = check_peaks(preds, cfg, k, maxpool, gpu)
    if maxpool and k == 24:
        assert np.array_equal(got["boxes"].cpu().numpy().view(np.int32), fix["decoded_topk_boxes"].view(np.int32))
    if maxpool and k == 50:      # the head of the longer list is the shorter list: the reference's boxes again
        assert np.array_equal(got["boxes"][:, :24].cpu().numpy().view(np.int32), fix["decoded_topk_boxes"].view(np.int32))


SMALL = {"single_cell": (1, 1, 1, 1, 1, 1), "every_cell_of_a_class": (2, 3, 5, 7, 35, 12), "rows_of_65": (2, 3, 3, 65, 50, 12),
         "rows_of_130": (2, 3, 3, 130, 50, 5), "rows_of_8_vector_form": (3, 2, 6, 8, 48, 32), "sixteen_classes": (1, 16, 4, 12, 40, 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SMALL))
def test_peaks_of_small_and_odd_maps(gpu, name):
    """(b), (c), (f): one cell; K = H * W, where suppressed zeros are chosen and the tie rule decides; rows that cross wave and
    16-byte boundaries with H * W no multiple of 4; rows of whole 16-byte groups (the vector form); the class and bin limits"""
    b, nc, h, w, k, bins = SMALL[name]
    check_peaks(random_maps(b, nc, h, w, bins, 3), cfg_with(rot_bins=bins), k, True, gpu)
    check_peaks(random_maps(b, nc, h, w, bins, 4), cfg_with(rot_bins=bins), k, False, gpu)


@pytest.mark.gpu
def test_peaks_on_plateaus_and_borders(gpu):
    """(d): equal values in 2 x 2 and 3 x 1 blocks (every cell of a plateau is a peak under ==), equal peaks of two classes at one cell,
    peaks in the four corners and on the four borders - equal ones among them, ordered by the index rule"""
    preds = random_maps(1, 2, 7, 9, 12, 5)
    hm = torch.full((1, 2, 7, 9), -1.0)
    hm[0, 0, 2:4, 2:4] = 2.0
    hm[0, 1, 1:4, 6] = 1.5
    hm[0, 0, 5, 6] = hm[0, 1, 5, 6] = 3.0
    for c, (y, x) in enumerate([(0, 0), (0, 8), (6, 0), (6, 8), (0, 4), (6, 4), (3, 0), (3, 8)]):
        hm[0, c % 2, y, x] = 2.5 if c < 4 else 2.0
    preds["hm"] = hm
    for k in (8, 17, 30, 63):
        got = check_peaks(preds, cfg_with(rot_bins=12), k, True, gpu)
    flat = (got["cls_id"].long() * 63 + got["cell"])[0].cpu()
    vals = got["cls"][0].gather(1, got["cls_id"][0].long().unsqueeze(1)).squeeze(1).cpu()
    assert vals[:2].tolist() == [3.0, 3.0] and flat[:2].tolist() == [5 * 9 + 6, 63 + 5 * 9 + 6]
    assert vals[2:6].tolist() == [2.5] * 4 and vals[6:14].tolist() == [2.0] * 8 and vals[14:17].tolist() == [1.5] * 3
    assert flat[2:6].tolist() == sorted(flat[2:6].tolist()) and flat[6:14].tolist() == sorted(flat[6:14].tolist())


@pytest.mark.gpu
def test_peaks_of_negative_maps_are_the_zeros_in_index_order(gpu):
    """(e): every logit negative: the zeros of the suppressed cells outrank every peak and come in index order"""
    preds = random_maps(2, 3, 9, 11, 12, 6)
    preds["hm"] = -preds["hm"].abs() - 0.1
    got = check_peaks(preds, cfg_with(rot_bins=12), 16, True, gpu)
    flat = (got["cls_id"].long() * 99 + got["cell"]).cpu()
    assert (flat[:, 1:] > flat[:, :-1]).all()
    picked = got["cls"].gather(2, got["cls_id"].long().unsqueeze(-1)).squeeze(-1)
    assert (picked == 0).all() and torch.signbit(picked).all()            # hm * 0.0 of a negative logit: -0.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["zeros_of_a_negative_map", "plateau_under_seven_peaks", "flat_4096", "flat_4160"])
def test_peaks_when_the_kth_value_is_shared_by_thousands(gpu, name):
    """The selection kernel sorts the candidates whole when at most 4096 keys lie in the k-th key's histogram bin or above it, and
    searches the k-th key bit by bit when more do: both sides of that size, and the search with many ties taken in index order."""
    if name == "zeros_of_a_negative_map":          # ~5300 zeros of suppressed cells outrank every (negative) peak
        preds, k = random_maps(1, 3, 40, 50, 12, 11), 20
        preds["hm"] = -preds["hm"].abs() - 0.1
    elif name == "plateau_under_seven_peaks":      # 7 peaks of 2.0, then the first 23 of ~4900 cells of 1.0 (each a peak under ==)
        preds, k = random_maps(1, 2, 50, 50, 12, 12), 30
        hm = torch.ones(1, 2, 50, 50)
        for c, y, x in [(0, 3, 3), (0, 20, 41), (0, 49, 49), (1, 0, 0), (1, 10, 10), (1, 30, 7), (1, 44, 25)]:
            hm[0, c, y, x] = 2.0
        preds["hm"] = hm
    else:                                          # one value everywhere: 4096 candidates are sorted, 4160 are searched
        w = 64 if name == "flat_4096" else 65
        preds, k = random_maps(1, 1, 64, w, 12, 13), 37
        preds["hm"] = torch.full((1, 1, 64, w), 0.75)
    got = check_peaks(preds, cfg_with(rot_bins=12), k, True, gpu)
    if name == "plateau_under_seven_peaks":
        flat = (got["cls_id"].long() * 2500 + got["cell"])[0].cpu().tolist()
        assert flat[:7] == [153, 1041, 2499, 2500, 3010, 4007, 4725] and flat[7:] == sorted(flat[7:]) and flat[7] == 0


@pytest.fixture(scope="module")
def kitti_maps():
    preds = random_maps(4, 3, 200, 176, 12, 8)
    assert best_are_distinct(np_heat(preds["hm"].numpy()), 50)
    return preds


@pytest.mark.gpu
def test_peaks_of_a_full_size_map(gpu, kitti_maps):
    """(g): 4 x 3 x 200 x 176, K = 50: many workgroups of keys, 26 strides of the selection loop"""
    check_peaks(kitti_maps, mm.MGAFConfig, 50, True, gpu)


@pytest.mark.gpu
def test_peaks_are_bit_identical_from_run_to_run_and_on_a_side_stream(gpu, kitti_maps):
    """(j)"""
    fix, cfg, preds = fixture()
    for maps, c, k in ((preds, cfg, 50), (kitti_maps, mm.MGAFConfig, 50)):
        on_dev = {n: t.to(gpu) for n, t in maps.items()}
        first = mm.center_peaks(on_dev, c, k)
        second = mm.center_peaks(on_dev, c, k)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            third = mm.center_peaks(on_dev, c, k)
        side.synchronize()
        for name, t in first.items():
            for other in (second, third):
                assert torch.equal(t.view(torch.int32) if t.dtype == torch.float32 else t, other[name].view(torch.int32) if t.dtype == torch.float32 else other[name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["k_zero", "k_above_cells", "k_513", "nc_17", "bins_33", "null_map"])
def test_bad_arguments_are_refused_before_any_launch(gpu, bad):
    """(i): FV2P_EINVAL (-1), and the outputs keep the pattern they were filled with"""
    b, nc, h, w, k, bins = 1, 3, 30, 20, 10, 12
    if bad == "nc_17":
        nc = 17
    if bad == "bins_33":
        bins = 33
    maps = [t.to(gpu) for t in (random_maps(b, nc, h, w, bins, 9)[n] for n in PEAK_MAPS)]
    k = {"k_zero": 0, "k_above_cells": h * w + 1, "k_513": 513}.get(bad, k)
    if bad == "null_map":
        maps[4] = None
    rows = max(k, 1)
    outs = [torch.full((b, rows, 7), 7.0, device=gpu), torch.full((b, rows, nc), 7.0, device=gpu), torch.full((b, rows), 7.0, device=gpu),
            torch.full((b, rows), 7, dtype=torch.int64, device=gpu), torch.full((b, rows), 7, dtype=torch.int32, device=gpu)]
    ws = torch.zeros(int(_nat.lib().fv2p_center_peaks_ws_bytes(b, nc, h, w)) + 256, dtype=torch.uint8, device=gpu)
    with pytest.raises(_nat.Fv2pError, match=r"fv2p_center_peaks failed \(-1\)"):
        _nat.call("fv2p_center_peaks", *maps, b, nc, h, w, k, 1, bins, 8, 0.05, 0.05, 0.0, -40.0, *outs, ws, ws.numel(), _nat.stream())
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in outs) and (ws == 0).all()


@pytest.mark.gpu
def test_sixteen_bit_maps_are_refused_in_python(gpu):
    preds = {n: t.to(gpu) for n, t in random_maps(1, 3, 4, 4, 12, 0).items()}
    preds["rot"] = preds["rot"].half()
    with pytest.raises(TypeError):
        mm.center_peaks(preds, mm.MGAFConfig, 4)


# ------------------------------------------------------------------ GPU tests: detections ----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", DETECTION_CASES)
def test_detections_equal_the_per_sample_composition(gpu, name):
    boxes, cls, loc, cfg, normalized, flags, want = detection_case(name, gpu)
    counts = check_detections(boxes, cls, loc, cfg, normalized, **flags)
    assert want(counts), counts


@pytest.mark.gpu
def test_detections_refuse_bad_arguments(gpu):
    boxes, cls, loc, cfg, *_ = detection_case("everything_passes", gpu)
    with pytest.raises(TypeError):
        mm.detections(boxes.half(), cls, loc, cfg)
    big = torch.zeros(1, 4097, 7, device=gpu)
    with pytest.raises(_nat.Fv2pError, match=r"\(-1\)"):
        mm.detections(big, torch.zeros(1, 4097, 3, device=gpu), torch.zeros(1, 4097, device=gpu), cfg)


# ------------------------------------------------------------------ GPU test: predict --------------------------------------------------
class _Recorder:
    """fv2p_native.call with the names of the entry points recorded."""

    def __init__(self, monkeypatch):
        self.names, real = [], _nat.call
        monkeypatch.setattr(_nat, "call", lambda name, *a: (self.names.append(name), real(name, *a))[1])


@pytest.mark.gpu
def test_predict_returns_the_detections_of_its_own_head_maps(gpu, monkeypatch):
    """MGAFDetector.predict on the reduced step of tests/test_mgaf_head.py (48 x 44 map, B = 2, random weights): the per-sample dicts are
    detections(center_peaks_tensor_ops(...)) of the head maps tapped from the same pass; after the head there are two library calls,
    one device-to-host copy (the counts) and no .item()."""
    from conftest import deterministic_libraries
    from test_mgaf_head import SmallMGAF, small_inputs
    torch.manual_seed(0)
    net = mm.MGAFDetector(SmallMGAF).to(gpu)
    feats, coords, _ = small_inputs()
    feats, coords = feats.to(gpu), coords.to(gpu)
    with deterministic_libraries(), torch.no_grad():
        # random weights: the yaml's 0.501 may pass nothing or everything.  The threshold of the run: in the widest gap between the 10th
        # and the 40th of sample 0's 50 sorted foreground scores, taken from a first pass
        first = net.head_maps(feats, coords, 2)
        peaks = mm.center_peaks_tensor_ops(first, SmallMGAF, SmallMGAF.num_inference_samples)
        fg = torch.sigmoid(peaks["cls"].double()).amax(-1)[0].sort()[0].cpu()
        gaps = fg[1:] - fg[:-1]
        at = 10 + int(gaps[10:40].argmax())
        assert gaps[at] > 1e-4, gaps[at]
        cfg = type("Cfg", (SmallMGAF,), {"score_thresh": float((fg[at] + fg[at + 1]) / 2)})
        net.cfg = cfg
        net.taps = {}
        out = net.predict(feats, coords, 2)
    preds = net.taps["preds"]
    peaks = mm.center_peaks_tensor_ops(preds, cfg, cfg.num_inference_samples)
    assert (torch.sigmoid(peaks["cls"].double()).amax(-1) - cfg.score_thresh).abs().min() > 1e-6
    want = mm.detections(peaks["boxes"], peaks["cls"], peaks["score"], cfg, normalized=False)
    want_counts = want["count"].cpu().tolist()
    assert 0 < want_counts[0] < 50

    rec = _Recorder(monkeypatch)
    syncs = {"cpu": 0, "item": 0, "tolist": 0, "numpy": 0, "nonzero": 0}
    for name in syncs:
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, _name=name, **kw):
            if self.is_cuda:
                syncs[_name] += 1
            return _real(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    again = net.detect(preds)
    assert rec.names == ["fv2p_center_peaks", "fv2p_detections_fgscore"], rec.names
    assert syncs == {"cpu": 1, "item": 0, "tolist": 0, "numpy": 0, "nonzero": 0}, syncs
    monkeypatch.undo()

    assert len(out) == 2 and len(again) == 2
    for i, d in enumerate(out):
        assert all(torch.equal(d[key], again[i][key]) for key in d)
        c = want_counts[i]
        assert sorted(d) == ["pred_boxes", "pred_labels", "pred_scores"]
        assert d["pred_boxes"].shape == (c, 7) and d["pred_scores"].shape == (c,) and d["pred_labels"].shape == (c,)
        assert torch.equal(d["pred_boxes"].view(torch.int32), want["boxes"][i, :c].contiguous().view(torch.int32))
        assert torch.equal(d["pred_scores"].view(torch.int32), want["scores"][i, :c].view(torch.int32))
        assert torch.equal(d["pred_labels"], want["labels"][i, :c].long())
        assert d["pred_labels"].dtype == torch.int64 and ((d["pred_labels"] >= 1) & (d["pred_labels"] <= 3)).all()
