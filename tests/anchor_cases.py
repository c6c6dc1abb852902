"""Cases for the first-stage kernels of csrc/targets.hip (fv2p_anchor_loss, fv2p_anchor_assign), shared by test_anchor_loss_gpu.py,
test_anchor_assign_gpu.py and test_anchor_cases_cpu.py (which checks the constructions themselves without a GPU).

Loss cases are dicts of float32 numpy arrays cls (B, A, 1), box (B, A, 7), dirs (B, A, 2), labels (B, A) int32, reg_t (B, A, 7),
anchor_rot (A), plus "meta" with what the construction promises.  Assign cases are dicts of gt (B, G, 8), anchors (A, 7), the
thresholds, the labels the rule gives by hand ("labels") and the anchors it forces ("forced": a set of (sample, anchor))."""
import math

import numpy as np
import torch

from fv2p_harness import fv2p_model as fm

CFG = fm.FV2PConfig
PI = math.pi
F32 = np.float32
BETA32 = F32(1.0 / 9.0)            # the kernel's beta: the C ABI takes 1 / 9 as a float
ROTS = (F32(0.0), F32(1.57))


# ------------------------------------------------------------------------------------------------ first-stage loss: the tensor form
def bare_head(anchor_rot, device, dtype, cfg=CFG):
    """An AnchorHead that holds what anchor_losses_tensor_ops reads: cfg and the anchors' headings."""
    head = fm.AnchorHead.__new__(fm.AnchorHead)
    torch.nn.Module.__init__(head)
    head.cfg = cfg
    anchors = np.zeros((anchor_rot.shape[0], 7), F32)
    anchors[:, 6] = anchor_rot
    head.register_buffer("anchors", torch.tensor(anchors, dtype=dtype, device=device))
    head.register_buffer("anchor_rot", torch.tensor(anchor_rot, dtype=dtype, device=device))
    return head


def tensors(case, device, dtype):
    t = {k: torch.tensor(case[k], dtype=dtype, device=device) for k in ("cls", "box", "dirs", "reg_t")}
    t["labels"] = torch.tensor(case["labels"], device=device)
    return t


def tensor_form(case, device, dtype, cfg=None):
    """anchor_losses_tensor_ops and autograd -> (loss, d cls, d box, d dirs) as float64 numpy."""
    cfg = cfg or case.get("cfg", CFG)
    t = tensors(case, device, dtype)
    leaves = [t[k].requires_grad_(True) for k in ("cls", "box", "dirs")]
    loss = bare_head(case["anchor_rot"], device, dtype, cfg).anchor_losses_tensor_ops(*leaves, t["labels"], t["reg_t"])
    grads = torch.autograd.grad(loss, leaves)
    return (float(loss.detach()),) + tuple(g.double().cpu().numpy() for g in grads)


def tensor_parts(case, device, dtype):
    """The three weighted terms of anchor_losses_tensor_ops, each from a run with the other two weights at 0."""
    parts = []
    for k in ("cls", "loc", "dir"):
        one = type("OnlyOneTerm", (CFG,), dict(rpn_w={j: (CFG.rpn_w[j] if j == k else 0.0) for j in CFG.rpn_w}))
        t = tensors(case, device, dtype)
        with torch.no_grad():
            parts.append(float(bare_head(case["anchor_rot"], device, dtype, one).anchor_losses_tensor_ops(t["cls"], t["box"], t["dirs"], t["labels"], t["reg_t"])))
    return parts


def dir_bins(ddirs):
    """The direction bin every anchor took, read from the sign pattern of d dirs (softmax minus one-hot: negative at the target bin,
    positive at the other); -1 where the anchor has no direction loss."""
    bins = np.full(ddirs.shape[:2], -1)
    bins[(ddirs[..., 0] < 0) & (ddirs[..., 1] > 0)] = 0
    bins[(ddirs[..., 1] < 0) & (ddirs[..., 0] > 0)] = 1
    return bins


# ------------------------------------------------------------------------------------------------ first-stage loss: cases
def alternating_rot(a):
    return np.array([ROTS[i % 2] for i in range(a)], F32)


def generic(b, a, seed, labels=None):
    """Logits N(0, 2), residuals on either side of beta, target headings over a full turn, labels a mix of 1, 0 and -1."""
    rng = np.random.default_rng(seed)
    reg_t = rng.normal(0, 0.5, (b, a, 7))
    reg_t[..., 6] = rng.uniform(-PI, PI, (b, a))
    box = reg_t + rng.normal(0, 0.15, (b, a, 7))
    box[..., 6] = reg_t[..., 6] + rng.normal(0, 0.5, (b, a))
    lab = rng.choice(np.array([1, 0, -1]), size=(b, a), p=[0.25, 0.55, 0.2]) if labels is None else labels
    case = dict(cls=rng.normal(0, 2, (b, a, 1)), box=box, dirs=rng.normal(0, 1, (b, a, 2)), reg_t=reg_t)
    case = {k: v.astype(F32) for k, v in case.items()}
    case.update(labels=np.asarray(lab).astype(np.int32).reshape(b, a), anchor_rot=alternating_rot(a), meta={})
    return case


def case_shape(b, a):
    c = generic(b, a, 1000 + 7 * b + a)
    c["labels"][0, 0] = 1
    return c


def no_positive_labels(rng, shape):
    return rng.choice(np.array([0, -1]), size=shape, p=[0.7, 0.3])


def case_no_positives_batch():
    c = generic(2, 300, 31)
    c["labels"][:] = no_positive_labels(np.random.default_rng(32), (2, 300))
    c["meta"]["no_positive_samples"] = [0, 1]
    return c


def case_no_positives_one_sample():
    c = generic(3, 257, 33)
    c["labels"][1] = no_positive_labels(np.random.default_rng(34), 257)
    c["meta"]["no_positive_samples"] = [1]
    return c


def case_all_ignored():
    c = generic(2, 257, 35)
    c["labels"][0] = -1
    c["meta"].update(no_positive_samples=[0], ignored_samples=[0])
    return c


def case_one_positive():
    c = generic(2, 257, 36)
    c["labels"][0] = no_positive_labels(np.random.default_rng(37), 257)
    c["labels"][0, 256] = 1                    # thread 0 of the second block, which holds this anchor only
    c["meta"]["positives"] = {0: 1}
    return c


def case_smooth_l1_edges():
    """All anchors positive.  Targets of 0 make the residual the prediction itself, exactly."""
    c = generic(1, 8, 38, labels=np.ones((1, 8)))
    below = np.nextafter(BETA32, F32(0))
    edges = [(0, 0, BETA32, "linear"), (1, 1, -BETA32, "linear"), (2, 2, F32(0), "zero"), (3, 3, below, "quadratic"), (4, 5, -below, "quadratic")]
    for a, j, v, _ in edges:
        c["reg_t"][0, a, j] = 0
        c["box"][0, a, j] = v
    c["box"][0, 5, 6] = c["reg_t"][0, 5, 6]    # sin(a) cos(a) - cos(a) sin(a): exactly 0 without contraction, chain cos(0) = 1
    c["meta"]["edges"] = edges + [(5, 6, F32(0), "zero")]
    return c


HEADING_DELTAS = (0.3, 2.0, -2.0, -0.3, PI / 2, -PI / 2, PI, -PI)


def case_headings():
    """box[6] - reg_t[6] in all four quadrants, and at +-pi/2 and +-pi where the chain factor cos(a - b) is 0 or -1."""
    n = len(HEADING_DELTAS)
    c = generic(1, n, 39, labels=np.ones((1, n)))
    c["reg_t"][0, :, 6] = np.linspace(-1.0, 1.0, n).astype(F32)
    c["box"][0, :, 6] = (c["reg_t"][0, :, 6].astype(np.float64) + np.array(HEADING_DELTAS)).astype(F32)
    return c


def fp32_bin_argument(x, rot, off):
    return F32(F32(x + rot) - off)             # reg_t[6] + anchor_rot - dir_offset, in that order


def heading_for(target, rot, off):
    """The float32 target heading x with fl(fl(x + rot) - off) == target, or, where no x gives it, the value nearest to the target
    on its side of 0."""
    target = F32(target)
    x = F32(F32(target + off) - rot)
    cands = [x]
    for _ in range(8):
        cands = [np.nextafter(cands[0], F32(-np.inf))] + cands + [np.nextafter(cands[-1], F32(np.inf))]
    vals = [fp32_bin_argument(v, rot, off) for v in cands]
    same_side = [i for i, v in enumerate(vals) if (v == target) or (target != 0 and np.sign(v) == np.sign(target))]
    best = min(same_side, key=lambda i: abs(float(vals[i]) - float(target)))
    return cands[best], vals[best]


PI32 = F32(PI)
# the value reg_t[6] + anchor_rot - dir_offset is to take, and the bin float32 gives it: v - floor(v / 2 pi) 2 pi, over pi, floored, clamped
BIN_TARGETS = (
    ("0", F32(0), 0),
    ("pi", PI32, 1),                                          # pi / pi = 1
    ("below pi", np.nextafter(PI32, F32(0)), 0),
    ("above pi", np.nextafter(PI32, F32(4)), 1),
    ("2 pi", F32(2 * PI), 0),                                 # floor(1) = 1: folds to 0
    ("-1e-8", F32(-1e-8), 1),                                 # v + 2 pi rounds to 2 pi: bin 2, clamped to 1
    ("-pi", -PI32, 1),                                        # -pi + 2 pi = pi
    ("3 pi", F32(3 * PI), 0),                                 # fl(3 pi) - fl(2 pi) rounds to just below fl(pi)
)


class QuarterPiOffset(CFG):
    """dir_offset = fl(pi / 4): with FV2PConfig's 0.78539 the sum lands midway between two floats near +-pi and rounding to even skips
    fl(pi) itself; with this offset every target but -1e-8 is met exactly."""
    dir_offset = float(F32(PI / 4))


def case_direction_bins(cfg=CFG):
    """Every target above under both anchor headings (0 and 1.57), all anchors positive; where no heading gives the target, the nearest
    value that can be had stands in.  -1e-8 never can: near dir_offset the sum moves in steps of 2^-24, so the nearest negative value,
    -2^-24, stands in for it (it takes the same way: lost when 2 pi is added)."""
    off = F32(cfg.dir_offset)
    n = 2 * len(BIN_TARGETS)
    c = generic(1, n, 40, labels=np.ones((1, n)))
    rows = []
    for i, (name, target, want) in enumerate(BIN_TARGETS):
        for k, rot in enumerate(ROTS):
            a = 2 * i + k
            assert c["anchor_rot"][a] == rot
            x, v = heading_for(target, rot, off)
            c["reg_t"][0, a, 6] = x
            rows.append((a, name, float(target), float(v), want))
    c["box"][0, :, 6] = c["reg_t"][0, :, 6] + F32(0.2)
    c["meta"]["bins"] = rows
    c["cfg"] = cfg
    return c


def case_saturated():
    c = generic(1, 16, 41)
    c["cls"][0, :8, 0] = (30.0, -30.0, 120.0, -120.0, 30.0, -30.0, 120.0, -120.0)
    c["labels"][0, :8] = (1, 1, 1, 1, 0, 0, 0, 0)
    return c


def case_zero_logits():
    c = generic(1, 16, 42)
    c["cls"][0, :3, 0] = 0.0
    c["labels"][0, :3] = (1, 0, -1)
    return c


class ThreeClassSmall(CFG):
    """FV2PConfig's three anchor entries and two rotations on a 6 x 5 BEV map: 180 anchors in (y, x, class, rotation) order."""
    point_cloud_range = (0.0, -8.0, -3.0, 16.0, 8.0, 1.0)
    grid_size = (48, 40, 40)


def case_three_class():
    """anchor_rot as a six-anchors-per-location head lays it out; per sample a positive on every (class, rotation) slot, with target
    headings in (-0.7, 0.7): there anchors of heading 0 take bin 1 and anchors of heading 1.57 take bin 0."""
    head = fm.AnchorHead(ThreeClassSmall, 4)
    rot = head.anchor_rot.numpy().astype(F32)
    a, nc, nr = rot.shape[0], len(CFG.anchor_classes), len(CFG.anchor_rotations)
    rng = np.random.default_rng(43)
    c = generic(2, a, 44, labels=no_positive_labels(rng, (2, a)))
    c["anchor_rot"] = rot
    slots = []
    for b in range(2):
        for s in range(nc * nr):
            idx = (7 * b + 5 * s + 3) % (a // (nc * nr)) * nc * nr + s
            c["labels"][b, idx] = s // nr + 1
            c["reg_t"][b, idx, 6] = F32(rng.uniform(-0.7, 0.7))
            slots.append((b, idx, 1 if rot[idx] == 0 else 0))
    c["meta"]["slots"] = slots
    return c


LOSS_CASES = {
    "shape_1x1": lambda: case_shape(1, 1), "shape_1x255": lambda: case_shape(1, 255), "shape_2x256": lambda: case_shape(2, 256),
    "shape_3x257": lambda: case_shape(3, 257), "shape_64x1100": lambda: case_shape(64, 1100),
    "no_positives_batch": case_no_positives_batch, "no_positives_one_sample": case_no_positives_one_sample, "all_ignored": case_all_ignored,
    "one_positive": case_one_positive, "smooth_l1_edges": case_smooth_l1_edges, "headings": case_headings,
    "direction_bins": case_direction_bins, "direction_bins_quarter_pi": lambda: case_direction_bins(QuarterPiOffset), "zero_logits": case_zero_logits, "three_class": case_three_class,
}
FP32_YARDSTICK = ("direction_bins", "direction_bins_quarter_pi")   # float64 folds some of these headings the other way


# ------------------------------------------------------------------------------------------------ target assignment: cases
MATCHED, UNMATCHED = 0.5, 0.25


def fp_box(x0, y0, x1, y1, cls, z=0.0, dz=1.5):
    """An axis-aligned, zero-heading box (8 values, class id last) with the footprint (x0, y0, x1, y1)."""
    return [(x0 + x1) / 2, (y0 + y1) / 2, z, x1 - x0, y1 - y0, dz, 0.0, float(cls)]


def fp_anchor(x0, y0, x1, y1, z=0.0, dz=1.5):
    return fp_box(x0, y0, x1, y1, 0, z, dz)[:7]


def footprint_iou(anchors, gt):
    """float32 IoU (A, G) of zero-heading footprints in numpy: the closed form the constructions are checked with."""
    def fp(b):
        return np.stack((b[:, 0] - b[:, 3] / 2, b[:, 1] - b[:, 4] / 2, b[:, 0] + b[:, 3] / 2, b[:, 1] + b[:, 4] / 2), 1).astype(F32)
    a, g = fp(anchors)[:, None], fp(gt)[None]
    inter = np.maximum(np.minimum(a[..., 2], g[..., 2]) - np.maximum(a[..., 0], g[..., 0]), 0) * \
        np.maximum(np.minimum(a[..., 3], g[..., 3]) - np.maximum(a[..., 1], g[..., 1]), 0)
    area = lambda f: (f[..., 2] - f[..., 0]) * (f[..., 3] - f[..., 1])
    return (inter / np.maximum(area(a) + area(g) - inter, F32(1e-6))).astype(F32)


def forced_set(case):
    """Anchors that attain a box's non-zero maximum, from footprint_iou."""
    out = set()
    for b in range(case["gt"].shape[0]):
        iou = footprint_iou(case["anchors"], case["gt"][b])
        top = iou.max(0)
        for a, j in zip(*np.nonzero((iou == top[None]) & (top[None] > 0))):
            out.add((b, int(a)))
    return out


def assign_case(samples, anchors, labels, forced, g=None, ious=()):
    g = g or max(len(s) for s in samples)
    gt = np.zeros((len(samples), g, 8), F32)
    for b, rows in enumerate(samples):
        for j, row in rows:
            gt[b, j] = row
    return dict(gt=gt, anchors=np.array(anchors, F32), matched=MATCHED, unmatched=UNMATCHED, labels=np.array(labels, np.int32).reshape(len(samples), -1),
                forced=set(forced), ious=list(ious))


def assign_thresholds():
    """Overlaps of exactly matched (0.5: positive, >=), exactly unmatched (0.25: ignored, < is strict) and 2 / 8.002 (background).  Each
    box also has an anchor identical to it, which takes the box's maximum: only those three are forced."""
    boxes = [(0, fp_box(0, 0, 2, 2, 1)), (1, fp_box(100, 0, 101, 2, 1)), (2, fp_box(200, 0, 201, 2, 1))]
    anchors = [fp_anchor(0, 0, 4, 2), fp_anchor(0, 0, 2, 2), fp_anchor(100, 0, 104, 2), fp_anchor(100, 0, 101, 2),
               fp_anchor(200, 0, 204.001, 2), fp_anchor(200, 0, 201, 2)]
    return assign_case([boxes], anchors, [1, 1, -1, 1, 0, 1], {(0, 1), (0, 3), (0, 5)},
                       ious=[(0, 0, 0, 0.5), (0, 2, 1, 0.25), (0, 1, 0, 1.0), (0, 3, 1, 1.0), (0, 5, 2, 1.0)])


def assign_forcing():
    """Anchors 0 and 1 share box 0's maximum of 0.25 (ignored unless forced): both forced.  Box 1's maximum is 0.125, below unmatched:
    anchor 2 is forced all the same.  Anchor 3 overlaps box 2 (class 2) by 0.375 and box 3 (class 1) by 0.25; anchor 4 is box 2 itself and
    takes its maximum, so anchor 3 is forced by box 3 alone, and takes the class and the regression target of box 2, its best box."""
    boxes = [(0, fp_box(0, 0, 2, 2, 1)), (1, fp_box(100, 0, 101, 2, 3)), (2, fp_box(200, 0, 201.5, 2, 2, z=0.5, dz=2.0)), (3, fp_box(203, 0, 204, 2, 1))]
    anchors = [fp_anchor(0, 0, 8, 2), fp_anchor(-6, 0, 2, 2), fp_anchor(100, 0, 108, 2), fp_anchor(200, 0, 204, 2), fp_anchor(200, 0, 201.5, 2)]
    case = assign_case([boxes], anchors, [1, 1, 3, 2, 2], {(0, 0), (0, 1), (0, 2), (0, 3), (0, 4)},
                       ious=[(0, 0, 0, 0.25), (0, 1, 0, 0.25), (0, 2, 1, 0.125), (0, 3, 2, 0.375), (0, 3, 3, 0.25), (0, 4, 2, 1.0)])
    case["best_box"] = {(0, 3): 2}
    return case


def assign_ties():
    """Sample 0: boxes 0 and 2 identical but for the class (the first wins), a zero row between them, box 3 that no anchor overlaps
    (forces nothing), box 4 of zero height under anchor 2 (its target meets the 1e-5 clamp; a box of zero footprint overlaps nothing
    and can never be matched).  Anchor 1 overlaps nothing.  Sample 1 is padding only."""
    boxes = [(0, fp_box(0, 0, 2, 2, 1)), (2, fp_box(0, 0, 2, 2, 2)), (3, fp_box(500, 500, 502, 502, 1)), (4, fp_box(300, 0, 304, 2, 1, dz=0.0))]
    anchors = [fp_anchor(0, 0, 2, 2), fp_anchor(50, 50, 54, 52), fp_anchor(300, 0, 304, 2)]
    case = assign_case([boxes, []], anchors, [[1, 0, 1], [0, 0, 0]], {(0, 0), (0, 2)}, g=6,
                       ious=[(0, 0, 0, 1.0), (0, 0, 2, 1.0), (0, 0, 1, 0.0), (0, 2, 4, 1.0)])
    case["best_box"] = {(0, 0): 0, (0, 2): 4}
    return case


def assign_shape(g, n_anchor, batch, seed):
    """n_anchor anchors of 4 x 2 on a row grid under both rotations; per sample a few boxes of classes 1..3 in rows spread over the whole
    padded list (so beyond row 256 where g allows), the rest padding; every sample has other boxes."""
    rng = np.random.default_rng(seed)
    idx = np.arange(n_anchor)
    anchors = np.zeros((n_anchor, 7), F32)
    anchors[:, 0], anchors[:, 1] = (idx % 40) * 3.0, (idx // 40) * 2.5
    anchors[:, 2:6] = (0.0, 4.0, 2.0, 1.5)
    anchors[:, 6] = alternating_rot(n_anchor)
    gt = np.zeros((batch, g, 8), F32)
    for b in range(batch):
        rows = sorted({0, g // 2, g - 1} | set(rng.integers(0, g, 5).tolist())) if g > 1 else [0]
        for j in rows:
            a = anchors[rng.integers(0, n_anchor)]
            size = (4.0, 2.0) if rng.uniform() < 0.5 else (2.0, 4.0)
            gt[b, j] = (a[0] + rng.normal(0, 0.6), a[1] + rng.normal(0, 0.4), rng.normal(0, 0.2), size[0] * rng.uniform(0.8, 1.2),
                        size[1] * rng.uniform(0.8, 1.2), rng.uniform(1.2, 1.8), rng.uniform(-PI, PI), rng.integers(1, 4))
    return dict(gt=gt, anchors=anchors, matched=0.6, unmatched=0.45)


ASSIGN_SHAPES = [(1, 1, 1), (48, 255, 3), (300, 257, 3), (1024, 1000, 1), (300, 1000, 3), (1024, 257, 1)]


def assign_reuse():
    """Two calls of one shape: boxes that are their anchors (maxima of 1.0), then the boxes of assign_forcing's kind that reach 0.25 and
    0.125 only.  With the first call's maxima left in the table nothing attains a maximum in the second: no anchor would be forced."""
    anchors = [fp_anchor(0, 0, 8, 2), fp_anchor(100, 0, 108, 2), fp_anchor(200, 0, 204, 2)]
    first = assign_case([[(0, fp_box(0, 0, 8, 2, 1)), (1, fp_box(100, 0, 108, 2, 2))]], anchors, [1, 2, 0], {(0, 0), (0, 1)}, g=2)
    second = assign_case([[(0, fp_box(0, 0, 2, 2, 1)), (1, fp_box(100, 0, 101, 2, 2))]], anchors, [1, 2, 0], {(0, 0), (0, 1)}, g=2,
                         ious=[(0, 0, 0, 0.25), (0, 1, 1, 0.125)])
    return first, second


ASSIGN_CASES = {"thresholds": assign_thresholds, "forcing": assign_forcing, "ties": assign_ties}


def assign_tensor_form(case, device):
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=device)
    anchors = t(case["anchors"])
    lab, reg = fm.AnchorHead.assign_one_tensor_ops(t(case["gt"]), anchors, fm.nearest_bev_boxes(anchors), case["matched"], case["unmatched"])
    return lab.cpu().numpy(), reg.cpu().numpy()


def encode64(box, anchor):
    """ResidualCoder's target of one box against one anchor, in float64."""
    box, anchor = np.asarray(box, np.float64), np.asarray(anchor, np.float64)
    a_sz, b_sz = np.maximum(anchor[3:6], 1e-5), np.maximum(box[3:6], 1e-5)
    diag = math.hypot(a_sz[0], a_sz[1])
    return np.concatenate(((box[:2] - anchor[:2]) / diag, (box[2:3] - anchor[2:3]) / a_sz[2], np.log(b_sz / a_sz), box[6:7] - anchor[6:7]))


def three_class_scene(head, device):
    """gt (2, 8, 8) for a three-class head: boxes of classes 1, 2 and 3 of their anchor's size, near anchor centres, under both headings;
    sample 1 has no box of class 3."""
    cfg = head.cfg
    rng = np.random.default_rng(45)
    gt = np.zeros((2, 8, 8), F32)
    centres = head.anchors_c0.cpu().numpy()[::2, :2]
    for b in range(2):
        j = 0
        for c, (size, bottom, _, _) in enumerate(cfg.anchor_classes):
            if b == 1 and c == 2:
                continue
            for k in range(2):
                x, y = centres[rng.integers(0, len(centres))]
                gt[b, j] = (x + rng.normal(0, 0.15), y + rng.normal(0, 0.15), bottom + size[2] / 2 + rng.normal(0, 0.1), size[0] * rng.uniform(0.9, 1.1),
                            size[1] * rng.uniform(0.9, 1.1), size[2], (0.0, 1.57)[k] + rng.normal(0, 0.1), c + 1)
                j += 1 + (b == 0 and c == 0 and k == 0)          # a zero row after the first box of sample 0
    return torch.from_numpy(gt).to(device)
