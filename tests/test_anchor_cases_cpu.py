"""CPU: the constructions of tests/anchor_cases.py hold what the GPU suites of fv2p_anchor_loss and fv2p_anchor_assign rely on - the
positives per sample, the smooth-L1 branch of every edge residual, the direction bin float32 gives every boundary heading (and that
float64 gives another to some: the reason those are held to the fp32 tensor form as well), the exact overlaps and forced anchors of
the assignment cases - and no loss case is ill-conditioned: the fp32 and float64 tensor forms agree to 1e-6 but at the bin boundaries."""
import numpy as np
import pytest
import torch

import anchor_cases as ac

F32 = np.float32


@pytest.fixture(scope="module")
def forms():
    """(case, fp32 tensor form, float64 tensor form) on the CPU, computed once per case."""
    memo = {}

    def get(name):
        if name not in memo:
            case = ac.LOSS_CASES[name]()
            memo[name] = (case, ac.tensor_form(case, "cpu", torch.float32), ac.tensor_form(case, "cpu", torch.float64))
        return memo[name]
    return get


@pytest.mark.parametrize("name", sorted(ac.LOSS_CASES))
def test_loss_case_is_float32_exact_and_well_conditioned(forms, name):
    case, f32, f64 = forms(name)
    b, a = case["labels"].shape
    assert case["cls"].shape == (b, a, 1) and case["box"].shape == case["reg_t"].shape == (b, a, 7) and case["dirs"].shape == (b, a, 2)
    assert case["anchor_rot"].shape == (a,) and case["labels"].dtype == np.int32
    assert all(case[k].dtype == F32 for k in ("cls", "box", "dirs", "reg_t", "anchor_rot"))
    assert set(np.unique(case["anchor_rot"]).tolist()) <= {0.0, float(F32(1.57))}
    for k, (x, y) in zip(("loss", "d cls", "d box", "d dirs"), zip(f32, f64)):
        e = np.abs(np.asarray(x) - np.asarray(y)).max()
        print(f"{name} {k}: E(fp32 cpu, float64) {e:.3e}  max {np.abs(np.asarray(y)).max():.3e}")
        assert np.isfinite(e)
        # E of the issue is that of the gradients; the loss (a sum over up to 70400 anchors, normalised by 1 without positives) is held
        # relative to its size, as everywhere in the project
        assert e < 1e-6 * (max(1.0, abs(y)) if k == "loss" else 1.0) or name in ac.FP32_YARDSTICK, (name, k, e)


@pytest.mark.parametrize("name", sorted(ac.LOSS_CASES))
def test_loss_case_positives_per_sample(forms, name):
    case, f32, _ = forms(name)
    pos = (case["labels"] > 0).sum(1)
    meta = case["meta"]
    print(f"{name}: positives per sample {pos.tolist()[:8]}")
    for smp in meta.get("no_positive_samples", []):
        assert pos[smp] == 0
        assert (f32[2][smp] == 0).all() and (f32[3][smp] == 0).all()
    for smp in meta.get("ignored_samples", []):
        assert (case["labels"][smp] == -1).all() and (f32[1][smp] == 0).all()
    for smp, n in meta.get("positives", {}).items():
        assert pos[smp] == n
    others = [s for s in range(len(pos)) if s not in meta.get("no_positive_samples", [])]
    assert all(pos[s] > 0 for s in others)
    if name.startswith("shape_"):
        assert {1, 0, -1} == set(np.unique(case["labels"]).tolist()) or case["labels"].size == 1
    if name in ("smooth_l1_edges", "headings") + ac.FP32_YARDSTICK:
        assert (case["labels"] == 1).all()
    if name == "one_positive":
        assert case["labels"][0, 256] == 1 and case["labels"].shape[1] == 257
    if name == "zero_logits":
        assert (case["cls"][0, :3, 0] == 0).all() and case["labels"][0, :3].tolist() == [1, 0, -1]
    if name == "three_class":
        assert sorted(set(case["labels"][case["labels"] > 0].tolist())) == [1, 2, 3]


def test_smooth_l1_edges_take_the_branches_they_are_built_for(forms):
    case, f32, f64 = forms("smooth_l1_edges")
    unit = ac.CFG.rpn_w["loc"] / 8.0          # one sample, eight positives
    for a, j, v, branch in case["meta"]["edges"]:
        if j < 6:
            d = case["box"][0, a, j] - case["reg_t"][0, a, j]
            assert d == v and d.dtype == F32
        else:
            assert case["box"][0, a, 6] == case["reg_t"][0, a, 6]
            d = F32(0)
        n = abs(d)
        assert {"linear": n >= ac.BETA32 and float(n) >= 1.0 / 9.0, "quadratic": 0 < n < ac.BETA32 and float(n) < 1.0 / 9.0, "zero": n == 0}[branch]
        for form in (f32, f64):
            g = form[2][0, a, j]
            print(f"edge anchor {a} channel {j}: residual {float(d):+.9e} {branch}: d box {g:+.9e}")
            if branch == "linear":
                assert abs(g - np.sign(d) * unit) < 1e-7
            elif branch == "zero":
                assert g == 0
            else:
                assert abs(g - float(d) * 9.0 * unit) < 1e-6 and abs(g) < unit
    assert abs(f32[2][0, 0, 0]) == F32(unit) and abs(f32[2][0, 1, 1]) == F32(unit)   # exactly at beta: the linear branch's +-1, no d / beta


@pytest.mark.parametrize("case_name,skipped", [("direction_bins", {"-1e-8", "pi", "-pi"}), ("direction_bins_quarter_pi", {"-1e-8"})])
def test_direction_bin_boundaries_fold_in_float32_as_built_and_otherwise_in_float64(forms, case_name, skipped):
    """`skipped`: the targets no float32 heading gives under that dir_offset (the nearest value stands in)."""
    case, f32, f64 = forms(case_name)
    bins32, bins64 = ac.dir_bins(f32[3])[0], ac.dir_bins(f64[3])[0]
    off = F32(case["cfg"].dir_offset)
    differ, exact = 0, {}
    for a, name, target, v, want in case["meta"]["bins"]:
        got_v = ac.fp32_bin_argument(case["reg_t"][0, a, 6], case["anchor_rot"][a], off)
        print(f"anchor {a} rot {case['anchor_rot'][a]:.2f} target {name} ({target:+.9e}): argument {float(got_v):+.9e}  bin fp32 {bins32[a]} float64 {bins64[a]}")
        assert float(got_v) == v and abs(v - target) <= 2.0 ** -21     # within two steps of the target where rounding to even skips it
        exact[name] = exact.get(name, False) or v == target
        if v == target or name == "-1e-8":
            assert bins32[a] == want, (a, name)
        differ += int(bins32[a] != bins64[a])
    assert {name for name, ok in exact.items() if not ok} == skipped, exact     # every other target is met exactly under one anchor heading at least
    v_small = [v for _, name, _, v, _ in case["meta"]["bins"] if name == "-1e-8"]
    assert all(-2.0 ** -23 < v < 0 for v in v_small)      # the stand-in for -1e-8: negative and lost when 2 pi is added
    assert (bins64 >= 0).all() and differ >= 1


def test_three_class_case_has_a_positive_on_every_slot_and_bins_that_follow_the_heading(forms):
    case, f32, f64 = forms("three_class")
    rot = case["anchor_rot"]
    assert rot.shape == (180,) and (rot.reshape(-1, 3, 2)[..., 0] == 0).all() and (rot.reshape(-1, 3, 2)[..., 1] == F32(1.57)).all()
    bins32, bins64 = ac.dir_bins(f32[3]), ac.dir_bins(f64[3])
    seen = set()
    for b, idx, want in case["meta"]["slots"]:
        assert case["labels"][b, idx] == (idx % 6) // 2 + 1
        assert bins32[b, idx] == want and bins64[b, idx] == want
        seen.add((b, idx % 6))
    assert seen == {(b, s) for b in range(2) for s in range(6)}
    assert ((bins32 >= 0) == (case["labels"] > 0)).all()


@pytest.mark.parametrize("name", sorted(ac.ASSIGN_CASES))
def test_assign_case_overlaps_forced_anchors_and_labels(name):
    case = ac.ASSIGN_CASES[name]()
    for b, a, j, want in case["ious"]:
        iou = ac.footprint_iou(case["anchors"], case["gt"][b])
        print(f"{name}: sample {b} anchor {a} box {j}: IoU {iou[a, j]!r}")
        assert iou[a, j] == F32(want)
    forced = ac.forced_set(case)
    print(f"{name}: forced {sorted(forced)}")
    assert forced == case["forced"] and len(forced) == {"thresholds": 3, "forcing": 5, "ties": 2}[name]
    labels, reg = ac.assign_tensor_form(case, "cpu")
    assert np.array_equal(labels, case["labels"])
    assert (reg[labels <= 0] == 0).all()
    for (b, a), j in case.get("best_box", {}).items():
        want = ac.encode64(case["gt"][b, j, :7], case["anchors"][a])
        assert np.abs(reg[b, a] - want).max() < 1e-6, (b, a, reg[b, a], want)


def test_assign_reuse_second_call_is_forced_only():
    first, second = ac.assign_reuse()
    assert first["gt"].shape == second["gt"].shape and np.array_equal(first["anchors"], second["anchors"])
    for case in (first, second):
        assert ac.forced_set(case) == case["forced"]
        assert np.array_equal(ac.assign_tensor_form(case, "cpu")[0], case["labels"])
    iou1, iou2 = ac.footprint_iou(first["anchors"], first["gt"][0]), ac.footprint_iou(second["anchors"], second["gt"][0])
    assert (iou1.max(0) == 1).all() and iou2.max(0).tolist() == [0.25, 0.125]      # every maximum falls: a stale table forces nothing
    assert (iou2.max(1) < second["matched"]).all()


@pytest.mark.parametrize("g,n_anchor,batch", ac.ASSIGN_SHAPES)
def test_assign_shape_cases_hold_every_label_kind(g, n_anchor, batch):
    case = ac.assign_shape(g, n_anchor, batch, 50 + g + n_anchor)
    assert case["gt"].shape == (batch, g, 8) and case["anchors"].shape == (n_anchor, 7)
    real = (case["gt"][..., 3] > 0).sum(1)
    assert (real >= 1).all() and (real <= 8).all()
    if g > 256:
        assert (case["gt"][:, 257:, 3] > 0).any(), "a box beyond the first 256 rows"
    labels, _ = ac.assign_tensor_form(case, "cpu")
    print(f"g {g} anchors {n_anchor} batch {batch}: boxes {real.tolist()} labels {[(int(v), int((labels == v).sum())) for v in np.unique(labels)]}")
    assert (labels > 0).any()
    if batch > 1:
        assert not np.array_equal(case["gt"][0], case["gt"][1])
