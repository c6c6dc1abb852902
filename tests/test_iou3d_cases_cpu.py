"""CPU: the iou3d oracle (oracle/iou3d_oracle.c) on the constructed inputs of tests/iou3d_cases.py against a float64 polygon clip, the
constructions the GPU suite (test_iou3d_edges_gpu.py) relies on - survivor lists in closed form, gate pairs on the side of the gate they
say - and the premise of the NMS pre-test of csrc/iou3d.hip: no pair with a non-empty reference polygon lies beyond its reach."""
import numpy as np
import pytest

import iou3d_cases as ic
import oracle
from boxes_util import exact_overlap


@pytest.fixture(scope="module")
def fams():
    return ic.families()


@pytest.fixture(scope="module")
def gates():
    pairs, meta = ic.gate_pairs()
    ov = np.array([oracle.boxes_bev(p[:1], p[1:], "overlap")[0, 0] for p in pairs])
    return pairs, meta, ov


def test_families_are_the_sizes_they_say_and_the_oracle_is_finite_on_them(fams):
    assert set(fams) == {"coincident", "touch", "aspect", "far", "yaw", "zero", "zero_crossing", "tiny0.003", "tiny0.01", "tiny0.03"}
    for name, b in fams.items():
        assert b.dtype == np.float32 and b.shape[1] == 7 and 11 <= b.shape[0] <= 40, name
        for other in (b, ic.partner_cars(name)):
            for mode in ("overlap", "iou"):
                assert np.isfinite(oracle.boxes_bev(b, other, mode)).all(), (name, mode)
                assert np.isfinite(oracle.boxes_bev(other, b, mode)).all(), (name, mode)
            assert np.isfinite(oracle.boxes_iou3d(b, other)).all()
    assert np.abs(fams["yaw"][:, 6]).min() >= 6 and np.abs(fams["yaw"][:, 6]).max() > 4000 and (fams["yaw"][:, 6] < 0).any()
    assert np.abs(fams["far"][:, :2]).min() > 990
    t = fams["touch"]
    assert t.shape[0] == 1 + 3 * len(ic.TOUCH_GAPS) and (t[:, 3:5] == 2).all() and (t[25:, 6] == np.float32(np.pi / 4)).all()


@pytest.mark.parametrize("name", ic.CLIP_FAMILIES)
def test_oracle_against_the_exact_clip(fams, name):
    """|oracle overlap - float64 intersection| <= 1e-2 (dx_a + dy_a + dx_b + dy_b + 4e-2) for every pair of the family: the reference's
    corner margin times the two half-perimeters."""
    b = fams[name]
    ov = oracle.boxes_bev(b, b, "overlap")
    exact = np.array([[exact_overlap(p, q) for q in b] for p in b])
    share = np.abs(ov.astype(np.float64) - exact) / ic.overlap_bound(b, b)
    i, j = np.unravel_index(np.argmax(share), share.shape)
    print(f"{name}: {b.shape[0]} x {b.shape[0]} pairs, overlapping {int((exact > 0).sum())}, worst share of the bound {share.max():.3g} "
          f"(pair {i}, {j}: oracle {ov[i, j]:.6g} exact {exact[i, j]:.6g})")
    assert share.max() <= 1.0
    assert (exact > 0).sum() > b.shape[0]          # more than the diagonal overlaps


def test_zero_extent_rows_have_no_overlap(fams):
    """exact_overlap divides by zero on a flat box, so no float64 clip here.  In the zero family the oracle is finite and exactly 0 wherever
    a box has no area.  Where flat rows cross whole boxes (zero_crossing, and either family against scattered cars) the reference finds
    every crossing twice and sums a sliver: measured here up to 1.0e-7 m^2 in one argument order and 0 in the other; such pairs are held
    to the corner-margin bound around the exact area, 0."""
    for name in ("zero", "zero_crossing"):
        b = fams[name]
        assert (b[4:7, 3] == 0).all() and (b[7:10, 4] == 0).all() and (b[10:13, 3:5] == 0).all() and (b[13:] == 0).all() and (b[:4, 3:5] > 1).all()
        assert (b[4:13, 3:5].max(1) > 0).sum() == 6 and (b[4:13, 5] > 0).all()
        flat = (b[:, 3] * b[:, 4]) == 0
        assert flat.sum() == 12 and not flat[ic.ZERO_WHOLE].any() and flat[ic.ZERO_FLAT].all()
        for other in (b, ic.partner_cars(name)):
            for x, y, rows in ((b, other, True), (other, b, False)):
                ov, iou = oracle.boxes_bev(x, y, "overlap"), oracle.boxes_bev(x, y, "iou")
                assert np.isfinite(ov).all() and np.isfinite(iou).all()
                mine = ov[flat] if rows else ov[:, flat]
                bound = ic.overlap_bound(x, y)[flat] if rows else ic.overlap_bound(x, y)[:, flat]
                print(f"{name} {'x' if other is b else 'x cars,'} flat {'rows' if rows else 'columns'}: nonzero {int((mine != 0).sum())} of {mine.size}, largest {mine.max():.3g}")
                assert (mine <= bound).all()
                if name == "zero" and other is b:
                    assert (mine == 0).all() and ((iou[flat] if rows else iou[:, flat]) == 0).all()
        assert (oracle.boxes_bev(b[:4], b[:4], "overlap") > 0).sum() > 4      # whole boxes do overlap each other
    cross = oracle.boxes_bev(fams["zero_crossing"], fams["zero_crossing"], "overlap")
    assert (cross[4:10, :4] != 0).any()                                       # and there the slivers do occur


def test_tiny_families_sit_in_the_margin_regime(fams):
    """Where the corner margin is larger than the boxes no float64 comparison is possible: finite values only, and IoUs above 1 do occur."""
    for s in ic.TINY_SCALES:
        b = fams[f"tiny{s:g}"]
        iou = oracle.boxes_bev(b, b, "iou")
        off = ~np.eye(b.shape[0], dtype=bool)
        print(f"tiny {s:g}: largest footprint side {b[:, 3:5].max():.4f}, pairs with IoU > 1: {int((iou[off] > 1).sum())}, largest IoU {iou[off].max():.3g}")
        assert np.isfinite(iou).all() and (b[:, 3:5] <= 2 * s * (1 + 1e-6)).all() and (b[:, 3:5] >= 0.5 * s * (1 - 1e-6)).all()
        if s <= ic.CORNER_MARGIN:
            assert (iou[off] > 1).any()


def test_library_host_entry_equals_the_oracle(fams, gates):
    """boxes_bev_iou_cpu (fv2p_boxes_iou_bev_cpu) runs the library's box_overlap, early-out included, on the host: bit for bit the oracle on
    every family against itself and against car boxes, and on the gate pairs (every first box against every second)."""
    from pcdet.ops.iou3d_nms import iou3d_nms_utils
    sets = [(name, b, b) for name, b in fams.items()] + [(name + " x cars", b, ic.partner_cars(name)) for name, b in fams.items()]
    sets.append(("gates", np.ascontiguousarray(gates[0][:, 0]), np.ascontiguousarray(gates[0][:, 1])))
    skipped = 0
    for name, a, b in sets:
        got = iou3d_nms_utils.boxes_bev_iou_cpu(a, b)
        assert got.dtype == np.float32 and np.array_equal(got, oracle.boxes_bev(a, b, "iou")), name
        d2 = (a[:, None, 0].astype(np.float64) - b[None, :, 0]) ** 2 + (a[:, None, 1].astype(np.float64) - b[None, :, 1]) ** 2
        skipped += int((d2 > ic.early_out_d2(a[:, None], b[None, :])).sum())
    assert skipped > 1000          # pairs the early-out answers do occur


# ------------------------------------------------------------------------------------------------ NMS structures
def descending(n):
    return -np.arange(n, dtype=np.float32)


@pytest.mark.parametrize("n", ic.NMS_SIZES + (3,))
def test_structures_hold_their_survivor_lists(n):
    for name, (boxes, thresh, want, flat) in ic.structures(n).items():
        assert boxes.shape == (n, 7) and boxes.dtype == np.float32
        got = oracle.nms(boxes, descending(n), thresh)
        assert np.array_equal(got, want), (name, n, got, want)
        if flat:
            assert (boxes[:, 6] == 0).all()
            assert np.array_equal(oracle.nms(boxes, descending(n), thresh, normal=True), want), (name, n)
    s = ic.structures(n)
    assert len(s["identical"][2]) == 1 and len(s["disjoint"][2]) == n and s["chain"][2].tolist() == list(range(0, n, 2))


def test_chain_neighbours_are_a_quarter_and_ghosts_sit_at_the_tile_boundary():
    boxes, _ = ic.chain(5)
    iou = oracle.boxes_bev(boxes, boxes, "iou")
    assert np.abs(np.diag(iou, 1) - 0.25).max() < 1e-6 and (np.diag(iou, 2) == 0).all()
    assert ic.ghost_indices(65, False) == (62, 63, 64) and ic.ghost_indices(193, True) == (0, 63, 192) and ic.ghost_indices(129, False) == (62, 63, 64)
    for n, last in ((65, False), (193, True)):
        boxes, want = ic.ghost(n, last)
        a, b, c = ic.ghost_indices(n, last)
        iou = oracle.boxes_bev(boxes[[a, b, c]], boxes[[a, b, c]], "iou")
        assert iou[0, 1] > 0.2 and iou[1, 2] > 0.2 and iou[0, 2] == 0          # A - B and B - C suppress, A - C does not touch
        assert b not in want and c in want and len(want) == n - 1
        rest = np.delete(np.arange(n), [a, b, c])
        assert (oracle.boxes_bev(boxes[rest], boxes, "overlap")[:, [a, b, c]] == 0).all()
    boxes, want = ic.far_column(193)
    assert sorted(set(range(193)) - set(want.tolist())) == [192] and np.array_equal(boxes[192], boxes[0])
    boxes, want = ic.far_column(129)
    assert sorted(set(range(129)) - set(want.tolist())) == [128]
    boxes, want = ic.far_column(127)
    assert sorted(set(range(127)) - set(want.tolist())) == [64, 126]


def test_threshold_edge_is_exactly_a_half():
    boxes, at, below = ic.threshold_edge(2)
    assert oracle.boxes_bev(boxes[:1], boxes[1:], "iou")[0, 0] == np.float32(0.5)
    assert float(ic.EDGE_THRESH_BELOW) < 0.5 == float(ic.EDGE_THRESH) and np.float32(0.5) - ic.EDGE_THRESH_BELOW < 1e-7
    assert at.tolist() == [0, 1] and below.tolist() == [0]


def test_batch_case_samples_finish_in_different_chunks():
    """With max_keep = 2 the batched pass works through 1 + 4 + 16 + 1 row blocks of BATCH_N boxes: identical never finds a second survivor,
    disjoint and chain hold two after their first rows, the tiny and the car sample find theirs later."""
    n = ic.BATCH_N
    batch = ic.batch_case(n)
    assert batch.shape == (5, n, 7) and batch.dtype == np.float32 and (n + 63) // 64 == 22
    second = []
    for s in range(5):
        keep = oracle.nms(batch[s], descending(n), ic.BATCH_THRESH)
        second.append(int(keep[1]) if len(keep) > 1 else None)
        print(f"{ic.BATCH_SAMPLES[s]}: {len(keep)} survivors of {n}, the second is row {second[-1]}, the 64th row {int(keep[63]) if len(keep) > 63 else None}")
    assert second[0] is None and second[1] == 1 and second[2] == 2
    cars = oracle.nms(batch[4], descending(n), ic.BATCH_THRESH)
    tiny = oracle.nms(batch[3], descending(n), ic.BATCH_THRESH)
    assert len(cars) > 64 and cars[63] >= 64 and 2 <= len(tiny) < n         # 64 survivors need more than the first row block; tiny stops short of n


# ------------------------------------------------------------------------------------------------ the gates
def test_gate_pairs_fall_on_the_side_they_say(gates):
    pairs, meta, ov = gates
    d = ic.centre_distance(pairs)
    a, b = pairs[:, 0].astype(np.float64), pairs[:, 1].astype(np.float64)
    assert len(meta) == 2 * 2 * 2 * (2 + 2 * len(ic.CIRCLE_OFFSETS))
    outside_early = 0
    for k, m in enumerate(meta):
        if m["gate"] == "early":
            rel = d[k] ** 2 / ic.early_out_d2(a[k], b[k]) - 1
            assert np.sign(rel) == np.sign(m["offset"]) and abs(rel - m["offset"]) < 1e-4, (m, rel)
        else:
            off = d[k] - ic.circle_base(a[k], b[k])
            assert np.sign(off) == np.sign(m["offset"]) and abs(off - m["offset"]) < 2e-6, (m, off)      # float32 rounding of the centres: < 1e-6
        if d[k] ** 2 > ic.early_out_d2(a[k], b[k]):
            outside_early += 1
            assert ov[k] == 0, (m, ov[k])          # what the early-out skips is exactly 0 in the reference
    assert outside_early == 8
    # side-by-side pairs of the small boxes are closer than the corner margin: the reference finds a polygon between disjoint boxes
    small = [k for k, m in enumerate(meta) if m["size"] == "small" and m["arrangement"] == "side_by_side" and m["gate"] == "circle" and abs(m["offset"]) == 1e-4]
    assert len(small) == 4 and (ov[small] > 0).all()
    print("gate pairs with a non-empty reference polygon: " + ", ".join(f"{meta[k]['size']} {meta[k]['arrangement']} {meta[k]['offset']:+g}" for k in np.nonzero(ov > 0)[0]))


CIRCLE_EXTRA = 1.5e-2       # csrc/iou3d.hip, circles_apart: `reach = (ra + rb) * 1.001f + 1e-4f + 1.5e-2f` - keep the two equal


def test_no_overlapping_pair_is_apart_under_the_pre_test(fams, gates):
    """The premise of nms_tile's pre-test: a pair circles_apart drops has overlap exactly 0 in the reference.  Every family against itself
    and against car boxes, the 200-box tiny sets of the NMS tests and the gate pairs, with circles_apart restated in numpy float32."""
    sets = [(name, b, b) for name, b in fams.items()] + [(name + " x cars", b, ic.partner_cars(name)) for name, b in fams.items()]
    sets += [(f"tiny {s:g} x 200", ic.tiny(s, n=200), ic.tiny(s, n=200)) for s in ic.TINY_SCALES]
    pairs, meta, gate_ov = gates
    dropped, lost = 0, []
    for name, a, b in sets:
        ov = oracle.boxes_bev(a, b, "overlap")
        apart = ic.circles_apart_f32(a, b, CIRCLE_EXTRA)
        dropped += int(apart.sum())
        if (apart & (ov > 0)).any():
            lost.append((name, int((apart & (ov > 0)).sum()), int((ov > 0).sum())))
    for k, p in enumerate(pairs):
        apart = bool(ic.circles_apart_f32(p[:1], p[1:], CIRCLE_EXTRA)[0, 0])
        dropped += apart
        assert apart == (meta[k]["gate"] == "early" or meta[k]["offset"] > CIRCLE_EXTRA), meta[k]       # the side the float64 formula says
        if apart and gate_ov[k] > 0:
            lost.append((meta[k], 1, 1))
    print(f"pre-test with +{CIRCLE_EXTRA:g}: drops {dropped} pairs, of which with a non-empty polygon: {lost}")
    assert dropped > 1000 and not lost
