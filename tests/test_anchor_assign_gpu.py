"""fv2p_anchor_assign (csrc/targets.hip: AxisAlignedTargetAssigner for a batch in two launches) through AnchorHead.assign_one_kernel
against AnchorHead.assign_one_tensor_ops on the hand-built anchors and boxes of tests/anchor_cases.py: labels bit for bit, regression
targets within 1e-6, and against what the rule gives by hand (tests/test_anchor_cases_cpu.py checks those expectations on the CPU):
overlaps exactly at the two thresholds, forced anchors, ties, degenerate rows, every shape at which the launch changes, a second call on
the same workspace, and the class-by-class route of a three-class head."""
import numpy as np
import pytest
import torch

from fv2p_harness import fv2p_model as fm

import anchor_cases as ac
from glue_util import tensor_ops

pytestmark = pytest.mark.gpu


def both(case, gpu):
    """(labels, reg) of the kernel and of the tensor form on the GPU, as numpy."""
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=gpu)
    gt, anchors = t(case["gt"]), t(case["anchors"])
    bev = fm.nearest_bev_boxes(anchors).contiguous()
    lab_k, reg_k = fm.AnchorHead.assign_one_kernel(gt, anchors, bev, case["matched"], case["unmatched"])
    lab_t, reg_t = fm.AnchorHead.assign_one_tensor_ops(gt, anchors, bev, case["matched"], case["unmatched"])
    assert lab_k.dtype == torch.int32 and lab_k.shape == lab_t.shape and reg_k.shape == reg_t.shape
    return lab_k.cpu().numpy(), reg_k.cpu().numpy(), lab_t.cpu().numpy(), reg_t.cpu().numpy()


def agree(what, lab_k, reg_k, lab_t, reg_t):
    err = float(np.abs(reg_k - reg_t).max())
    print(f"{what}: labels {[(int(v), int((lab_k == v).sum())) for v in np.unique(lab_k)]}  max |reg kernel - reg tensor form| {err:.3e}")
    assert np.array_equal(lab_k, lab_t), what
    assert np.isfinite(reg_k).all() and err < 1e-6, what
    assert (reg_k[lab_k <= 0] == 0).all()


@pytest.mark.parametrize("name", sorted(ac.ASSIGN_CASES))
def test_anchor_assign_hand_built_cases(gpu, name):
    case = ac.ASSIGN_CASES[name]()
    forced = ac.forced_set(case)
    assert forced == case["forced"] and len(forced) == {"thresholds": 3, "forcing": 5, "ties": 2}[name]
    lab_k, reg_k, lab_t, reg_t = both(case, gpu)
    agree(name, lab_k, reg_k, lab_t, reg_t)
    print(f"{name}: kernel labels {lab_k.tolist()} by hand {case['labels'].tolist()} forced {sorted(forced)}")
    assert np.array_equal(lab_k, case["labels"])
    for (b, a), j in case.get("best_box", {}).items():
        want = ac.encode64(case["gt"][b, j, :7], case["anchors"][a])
        print(f"{name}: anchor {a} takes box {j}: target {reg_k[b, a]} float64 {want}")
        # against float64 by hand: 1e-6, or four float32 steps where the target is large (log(1e-5 / 1.5) = -11.9 has steps of 9.5e-7)
        assert (np.abs(reg_k[b, a] - want) <= np.maximum(1e-6, 4 * np.spacing(np.abs(want).astype(np.float32)))).all()
    if name == "ties":
        assert abs(reg_k[0, 2, 5] - np.log(1e-5 / 1.5)) < 4e-6, "a box of zero height: the target of the 1e-5 clamp"
        assert (lab_k[1] == 0).all()


@pytest.mark.parametrize("g,n_anchor,batch", ac.ASSIGN_SHAPES)
def test_anchor_assign_shapes(gpu, g, n_anchor, batch):
    """g up to the entry point's 1024 (beyond 256 the LDS fill loops stride), anchor counts off a multiple of the 256-thread workgroup, one
    and three samples with their own boxes; the boxes are spread over the whole padded list."""
    case = ac.assign_shape(g, n_anchor, batch, 50 + g + n_anchor)
    lab_k, reg_k, lab_t, reg_t = both(case, gpu)
    agree(f"g {g} anchors {n_anchor} batch {batch}", lab_k, reg_k, lab_t, reg_t)
    assert (lab_k > 0).any()


def test_anchor_assign_second_call_on_the_same_workspace(gpu):
    """The per-box maxima live in a workspace that every call shares: a second call whose boxes overlap less must not see the first one's."""
    first, second = ac.assign_reuse()
    lab1 = both(first, gpu)[0]
    lab_k, reg_k, lab_t, reg_t = both(second, gpu)
    agree("second call", lab_k, reg_k, lab_t, reg_t)
    print(f"first call {lab1.tolist()} second call {lab_k.tolist()} by hand {second['labels'].tolist()}")
    assert np.array_equal(lab1, first["labels"]) and np.array_equal(lab_k, second["labels"])
    # and in the larger table of a strided fill: many boxes first, then the same shape with fewer overlaps
    big = ac.assign_shape(300, 257, 3, 60)
    both(big, gpu)
    less = dict(big, gt=big["gt"].copy())
    less["gt"][..., 0] += 1.5
    agree("second call, g 300", *both(less, gpu))


def test_anchor_assign_three_class_route(gpu):
    """head.assign against head.assign_tensor_ops on FV2PConfig's three anchor entries over a 6 x 5 map: every class's anchors see the
    boxes of their own class only."""
    head = fm.AnchorHead(ac.ThreeClassSmall, 4).to(gpu)
    gt = ac.three_class_scene(head, gpu)
    assert sorted(set(gt[0, :, 7].tolist())) == [0.0, 1.0, 2.0, 3.0] and sorted(set(gt[1, :, 7].tolist())) == [0.0, 1.0, 2.0]
    lab, reg = head.assign(gt)
    with tensor_ops():
        lab_t, reg_t = head.assign(gt)
    lab_o, reg_o = head.assign_tensor_ops(gt)
    assert torch.equal(lab_t, lab_o) and torch.equal(reg_t, reg_o)
    agree("three classes", lab.cpu().numpy(), reg.cpu().numpy(), lab_t.cpu().numpy(), reg_t.cpu().numpy())
    per_class = lab.view(2, -1, 3, 2).cpu().numpy()
    for c in range(3):
        kinds = set(np.unique(per_class[:, :, c]).tolist())
        print(f"class {c + 1} anchors: labels {sorted(kinds)} positives per sample {(per_class[:, :, c] > 0).sum((1, 2)).tolist()}")
        assert kinds <= {-1, 0, c + 1}
        assert (per_class[0, :, c] == c + 1).any()
    assert (per_class[1, :, 2] == 0).all(), "sample 1 has no box of class 3"
    assert (per_class[1, :, :2] > 0).any()
