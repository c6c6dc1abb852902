"""Constructed inputs for the rotated-box IoU / NMS kernels of csrc/iou3d.hip.  numpy only, no project code.

The kernels hold three things the oracle (oracle/iou3d_oracle.c, the reference's arithmetic restated) does not have: the sqrt-free early-out
at the head of box_overlap, the bounding-circle pre-test of the NMS tiles (circles_apart) and the chunked, early-stopping greedy pass of
the batched NMS.  Random car-sized boxes reach none of their edges.  Here are box families at those edges (coincident and collinear edges,
gaps around the reference's 1e-2 corner margin, extreme aspect ratios, far-away centres, large headings, zero extents, footprints smaller
than the corner margin), pairs placed on either side of each shortcut's boundary, and NMS structures whose survivor list is known in
closed form at every tile size.

tests/test_iou3d_cases_cpu.py holds the oracle on these inputs to a float64 polygon clip and checks that every construction holds what it
says; tests/test_iou3d_edges_gpu.py holds the kernels to the oracle bit for bit."""
import numpy as np

F32 = np.float32
CAR = (3.9, 1.6, 1.56)
CORNER_MARGIN = 1e-2               # MARGIN of the reference's corner test (iou3d_nms_kernel.cu:53), per axis of the box frame


def _rows(xy, z, dims, yaw):
    n = len(yaw)
    return np.concatenate([np.asarray(xy, np.float64).reshape(n, 2), np.asarray(z, np.float64).reshape(n, 1),
                           np.asarray(dims, np.float64).reshape(n, 3), np.asarray(yaw, np.float64).reshape(n, 1)], 1).astype(F32)


def car_boxes(seed, n, centre=(0.0, 0.0), sigma=1.5):
    """n car-sized boxes (0.7 .. 1.3 of 3.9 x 1.6 x 1.56) scattered with `sigma` around `centre`, yaw in +-pi."""
    rng = np.random.default_rng(seed)
    return _rows(np.asarray(centre) + rng.normal(0, sigma, (n, 2)), rng.uniform(-1.5, 0.5, n), np.array(CAR) * rng.uniform(0.7, 1.3, (n, 3)),
                 rng.uniform(-np.pi, np.pi, n))


# ------------------------------------------------------------------------------------------------ box families
COINCIDENT_YAWS = (0.0, np.pi / 2, -np.pi / 2, np.pi, 2 * np.pi, 1e-4, -1e-4, np.pi / 2 + 1e-4, 0.5, 8 * np.pi + 0.5, 100.0)


def coincident():
    """One car box at eleven headings: the same rectangle (0, pi, 2 pi), its quarter turns, nearly parallel edges, a whole number of turns
    on top of 0.5 and a heading of 100 rad."""
    n = len(COINCIDENT_YAWS)
    return _rows(np.tile([1.0, -2.0], (n, 1)), np.full(n, -0.5), np.tile(CAR, (n, 1)), COINCIDENT_YAWS)


TOUCH_GAPS = (-1e-2, -1e-3, -1e-6, 0.0, 1e-6, 1e-3, 5e-3, 9.9e-3, 1e-2, 1.01e-2, 2e-2, 5e-2)
TOUCH_ARRANGEMENTS = ("along_x", "diagonal", "diamond")


def touch():
    """Row 0: a 2 x 2 box at the origin.  Then, for each arrangement, one partner per gap of TOUCH_GAPS (negative: the two overlap by that
    much): a 2 x 2 box shifted along x (edge to edge), one shifted along the diagonal (corner to corner, the gap measured along it) and a
    2 x 2 box at 45 degrees whose tip points at the middle of the right edge.  Row 1 + 12 a + g is arrangement a at gap g."""
    xy, yaw = [(0.0, 0.0)], [0.0]
    for g in TOUCH_GAPS:
        xy.append((2.0 + g, 0.0)), yaw.append(0.0)
    for g in TOUCH_GAPS:
        xy.append((2.0 + g / np.sqrt(2), 2.0 + g / np.sqrt(2))), yaw.append(0.0)
    for g in TOUCH_GAPS:
        xy.append((1.0 + np.sqrt(2) + g, 0.0)), yaw.append(np.pi / 4)
    n = len(yaw)
    return _rows(xy, np.zeros(n), np.tile([2.0, 2.0, 1.0], (n, 1)), yaw)


ASPECT_DX, ASPECT_DY = (100.0, 20.0, 0.2, 0.05), (30.0, 0.2, 0.05)


def aspect(seed=11):
    """Every dx of ASPECT_DX with every dy of ASPECT_DY, twice: walls, poles and slabs through one another, centres within +-3, any yaw."""
    rng = np.random.default_rng(seed)
    dims = np.array([(dx, dy, 1.5) for dx in ASPECT_DX for dy in ASPECT_DY] * 2)
    n = dims.shape[0]
    return _rows(rng.uniform(-3, 3, (n, 2)), rng.uniform(-0.5, 0.5, n), dims, rng.uniform(-np.pi, np.pi, n))


def far(seed=12, n=24):
    """Car boxes around (1000, -2000): a float32 step of the coordinates is 6e-5 .. 1.2e-4 m there."""
    return car_boxes(seed, n, centre=(1000.0, -2000.0), sigma=1.5)


def yaw(seed=13, n=24):
    """Car boxes with |yaw| uniform in [6, 8000] (fv2p_sinf / fv2p_cosf are specified to 8192), either sign."""
    rng = np.random.default_rng(seed)
    b = car_boxes(seed, n)
    b[:, 6] = (rng.uniform(6, 8000, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
    return b


ZERO_WHOLE, ZERO_FLAT = slice(0, 4), slice(4, 16)


def zero():
    """Sixteen rows: four whole boxes about one centre (a 3.9 x 1.6 box at heading 0.4, and it again 1.3, 1.2 and 1.1 times as large at
    headings 0.45, 0.35 and 0.4 + pi), then three rows each with dx = 0, dy = 0 and dx = dy = 0 and three all-zero padding rows.  The
    flat rows lie along the axes of the first box, well inside all four whole boxes and 0.3 m and more from one another; the padding rows sit
    at the origin, away from everything.  No edge of a flat row crosses another edge and no corner comes within the corner margin of
    another box's outline, so the reference's polygon of a pair with a flat row is a set of bitwise-equal points: overlap exactly 0."""
    cx, cy, h = 5.0, 3.0, 0.4
    c, s = np.cos(h), np.sin(h)
    place = lambda lx, ly: (cx + lx * c - ly * s, cy + lx * s + ly * c)
    rows = [(cx, cy, 0.0, 3.9 * k, 1.6 * k, 1.5, hh) for k, hh in ((1.0, h), (1.3, h + 0.05), (1.2, h - 0.05), (1.1, h + np.pi))]
    rows += [place(lx, 0.0) + (0.1, 0.0, 1.0, 1.5, h) for lx in (-0.9, -0.6, -0.3)]           # dx = 0: a segment along the box's y axis
    rows += [place(0.7, ly) + (-0.1, 0.8, 0.0, 1.5, h) for ly in (-0.2, 0.0, 0.2)]            # dy = 0: a segment along its x axis
    rows += [place(0.0, ly) + (0.0, 0.0, 0.0, 1.5, h) for ly in (-0.3, 0.0, 0.3)]             # a point
    rows += [(0.0,) * 7] * 3
    return np.array(rows, np.float64).astype(F32)


def zero_crossing(seed=14):
    """Sixteen car boxes scattered around one spot, four of them whole, then three each with dx = 0, dy = 0, dx = dy = 0 and three all-zero
    rows: here the flat rows do cross the whole boxes.  A crossing is found twice (once per coincident edge of the flat box, with the
    operands in the other order), so the reference's polygon is a sliver with an area of the order of a float32 rounding, not exactly 0."""
    b = car_boxes(seed, 16, sigma=0.8)
    b[4:7, 3] = 0
    b[7:10, 4] = 0
    b[10:13, 3:5] = 0
    b[13:] = 0
    return b


TINY_SCALES = (0.003, 0.01, 0.03)


def tiny(scale, n=40, seed=15):
    """Footprints of scale * U(0.5, 2), centres uniform in +-(3 scale + 0.03): at 0.003 and 0.01 the reference's corner margin is larger than
    the boxes, so disjoint boxes still have a non-empty polygon and IoUs above 1 occur."""
    rng = np.random.default_rng(seed + int(round(scale * 1e4)))
    half = 3 * scale + 0.03
    dims = np.concatenate([scale * rng.uniform(0.5, 2, (n, 2)), rng.uniform(1.0, 2.0, (n, 1))], 1)
    return _rows(rng.uniform(-half, half, (n, 2)), rng.uniform(-0.2, 0.2, n), dims, rng.uniform(-np.pi, np.pi, n))


def families():
    """name -> [n, 7] float32, 11 <= n <= 40."""
    out = dict(coincident=coincident(), touch=touch(), aspect=aspect(), far=far(), yaw=yaw(), zero=zero(), zero_crossing=zero_crossing())
    for s in TINY_SCALES:
        out[f"tiny{s:g}"] = tiny(s)
    return out


CLIP_FAMILIES = ("coincident", "touch", "aspect", "far", "yaw")     # those a float64 polygon clip can judge


def partner_cars(name, n=12):
    """Car boxes scattered over the family's own boxes (the second operand of 'family against car boxes')."""
    b = families()[name]
    centre = b[:, :2].astype(np.float64).mean(0)
    return car_boxes(100 + len(name), n, centre=centre, sigma=1.0)


def overlap_bound(a, b):
    """[na, nb]: what the reference's overlap may differ by from the exact intersection area.  A corner is accepted up to CORNER_MARGIN
    outside a box along each axis, so the polygon may grow by a strip of that width along the perimeter of both boxes (plus the four
    margin-sized corner squares): 1e-2 * (dx_a + dy_a + dx_b + dy_b + 4e-2)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return CORNER_MARGIN * ((a[:, 3] + a[:, 4])[:, None] + (b[:, 3] + b[:, 4])[None, :] + 4 * CORNER_MARGIN)


# ------------------------------------------------------------------------------------------------ the two shortcuts' gates
# csrc/iou3d.hip, box_overlap: returns 0 at once when  d^2 > 3 (ra^2 + rb^2 + 0.01)      (d: centre distance, r: half-diagonal)
# csrc/iou3d.hip, circles_apart: a pair is never evaluated when  d > reach,  reach = (ra + rb) * 1.001 + 1e-4 + CIRCLE_EXTRA
EARLY_OUT_REL = 1e-3                                   # pairs at d^2 = 3 (ra^2 + rb^2 + 0.01) (1 -+ 1e-3)
CIRCLE_OFFSETS = (1e-4, 5e-3, 1.4e-2, 2e-2)            # pairs at d = (ra + rb) 1.001 + 1e-4 -+ each of these


def half_diagonal(b):
    b = np.asarray(b, np.float64)
    return 0.5 * np.sqrt(b[..., 3] ** 2 + b[..., 4] ** 2)


def early_out_d2(a, b):
    return 3.0 * (half_diagonal(a) ** 2 + half_diagonal(b) ** 2 + 0.01)


def circle_base(a, b):
    """The reach of circles_apart without its allowance for the corner margin, float64."""
    return (half_diagonal(a) + half_diagonal(b)) * 1.001 + 1e-4


def gate_pairs():
    """-> (pairs [K, 2, 7] float32, meta: list of dict(gate, offset, size, arrangement, yaw)).  Two equal boxes with a common heading, car-sized
    (3.9 x 1.6) or 0.02-sized (0.02 x 0.02), the second placed from the first along the box diagonal (tip to tip: the corners face each
    other, the closest two disjoint boxes of these circles can be) or along the short side (side by side), at a centre distance worked out
    in float64 from the gate's formula: `early` pairs at d^2 = early_out_d2 * (1 + offset), offset -+1e-3; `circle` pairs at
    d = circle_base + offset, offset -+ each of CIRCLE_OFFSETS."""
    pairs, meta = [], []
    for size, (dx, dy) in (("car", (3.9, 1.6)), ("small", (0.02, 0.02))):
        for heading in (0.0, 0.7):
            a = np.array([0.5, -0.25, 0.0, dx, dy, 1.5, heading])
            c, s = np.cos(heading), np.sin(heading)
            for arrangement in ("tip_to_tip", "side_by_side"):
                u = np.array([dx, dy]) / np.hypot(dx, dy) if arrangement == "tip_to_tip" else np.array([0.0, 1.0])
                direction = np.array([u[0] * c - u[1] * s, u[0] * s + u[1] * c])
                dists = [("early", o, np.sqrt(early_out_d2(a, a) * (1 + o))) for o in (-EARLY_OUT_REL, EARLY_OUT_REL)]
                dists += [("circle", sign * o, circle_base(a, a) + sign * o) for o in CIRCLE_OFFSETS for sign in (-1.0, 1.0)]
                for gate, offset, d in dists:
                    b = a.copy()
                    b[:2] = a[:2] + d * direction
                    pairs.append(np.stack([a, b]))
                    meta.append(dict(gate=gate, offset=offset, size=size, arrangement=arrangement, yaw=heading))
    return np.stack(pairs).astype(F32), meta


def centre_distance(pairs):
    p = np.asarray(pairs, np.float64)
    return np.hypot(p[:, 0, 0] - p[:, 1, 0], p[:, 0, 1] - p[:, 1, 1])


def circles_apart_f32(a, b, extra):
    """[na, nb] bool: circles_apart of csrc/iou3d.hip restated operation for operation in numpy float32, with `extra` its allowance for
    the corner margin."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    dx, dy = a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1]
    ra = F32(0.5) * np.sqrt(a[:, 3] * a[:, 3] + a[:, 4] * a[:, 4])
    rb = F32(0.5) * np.sqrt(b[:, 3] * b[:, 3] + b[:, 4] * b[:, 4])
    reach = (ra[:, None] + rb[None, :]) * F32(1.001) + F32(1e-4) + F32(extra)
    return dx * dx + dy * dy > reach * reach


# ------------------------------------------------------------------------------------------------ NMS structures
# Boxes in score order (index 0 first).  Every builder returns (boxes [n, 7] float32, survivors in closed form).
NMS_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 193)


def _filler(n):
    """n car boxes on a lattice of 10 m pitch, 20 m and more away from the origin: none near another or near the placed boxes."""
    i = np.arange(n)
    return _rows(np.stack([10.0 * (i % 16), 20.0 + 10.0 * (i // 16)], 1), np.zeros(n), np.tile(CAR, (n, 1)), np.zeros(n))


def identical(n, heading=0.0):
    """n copies of one box: box 0 suppresses every other one (every word of its mask row is full)."""
    return _rows(np.tile([3.0, -1.0], (n, 1)), np.zeros(n), np.tile(CAR, (n, 1)), np.full(n, heading)), np.arange(min(n, 1))


def disjoint(n):
    return _filler(n), np.arange(n)


def chain(n):
    """2 x 2 boxes stepped 1.2 m along x: neighbours overlap by 0.8 x 2, IoU 1.6 / 6.4 = 0.25; second neighbours are 0.4 m apart.
    Above a threshold of 0.2 every odd box falls to the even one before it, across every tile boundary."""
    return _rows(np.stack([1.2 * np.arange(n), np.zeros(n)], 1), np.zeros(n), np.tile([2.0, 2.0, 1.0], (n, 1)), np.zeros(n)), np.arange(0, n, 2)


def _chain_link(k):
    return np.array([1.2 * k, 0.0, 0.0, 2.0, 2.0, 1.0, 0.0], F32)


def ghost_indices(n, c_last):
    """(a, b, c): b = 63 where n allows (the last row of tile 0), a the row before it (row 0 with c_last), c the row after it (the first row
    of tile 1) or, with c_last, the last row of the last tile."""
    b = max(min(63, n - 2), 0)
    a = 0 if c_last else max(b - 1, 0)
    c = n - 1 if c_last else b + 1
    return a, b, c


def ghost(n, c_last=False):
    """A suppresses B, B would suppress C, A does not touch C: C survives, because its only suppressor was itself suppressed.  Three links of
    the chain at rows ghost_indices(n, c_last), lattice boxes elsewhere.  With fewer than three rows only A (and B) exist."""
    boxes = _filler(n)
    a, b, c = ghost_indices(n, c_last)
    roles = [r for r in dict.fromkeys((a, b, c)) if r < n]
    for k, r in enumerate(roles):
        boxes[r] = _chain_link(k)
    gone = [roles[1]] if len(roles) > 1 else []
    return boxes, np.array([i for i in range(n) if i not in gone], np.int64)


def far_column(n):
    """Box 0 again at the first and at the last row of the last tile: box 0's only victims sit in the last column block."""
    boxes = _filler(n)
    victims = sorted({r for r in (64 * ((n - 1) // 64), n - 1) if r > 0})
    for r in victims:
        boxes[r] = boxes[0]
    return boxes, np.array([i for i in range(n) if i not in victims], np.int64)


EDGE_THRESH = F32(0.5)
EDGE_THRESH_BELOW = np.nextafter(F32(0.5), F32(0))


def threshold_edge(n):
    """Rows 0 and n - 1: a 2 x 2 box and a 2 x 1 box inside it, overlap 2, union 4, IoU exactly 0.5 in float32.  `>` decides: both survive at
    0.5, row n - 1 falls at the float32 below 0.5.  -> (boxes, survivors at 0.5, survivors just below)."""
    boxes = _filler(n)
    boxes[0] = [0, 0, 0, 2, 2, 1, 0]
    if n > 1:
        boxes[n - 1] = [0, 0.5, 0, 2, 1, 1, 0]
    return boxes, np.arange(n), np.arange(max(n - 1, 1))


def structures(n):
    """name -> (boxes, thresh, survivors, axis_aligned): axis-aligned structures have the same survivors under normal (heading-free) NMS."""
    edge, at, below = threshold_edge(n)
    out = {"identical": identical(n) + (0.5, True), "identical_turned": identical(n, 0.3) + (0.5, False), "disjoint": disjoint(n) + (0.0, True),
           "chain": chain(n) + (0.2, True), "ghost": ghost(n) + (0.2, True), "ghost_last_tile": ghost(n, True) + (0.2, True),
           "far_column": far_column(n) + (0.5, True)}
    out = {k: (b, F32(t), s, flat) for k, (b, s, t, flat) in out.items()}
    out["threshold_edge_at"] = (edge, EDGE_THRESH, at, True)
    out["threshold_edge_below"] = (edge, EDGE_THRESH_BELOW, below, True)
    return out


# ------------------------------------------------------------------------------------------------ the batched call
BATCH_N = 1345          # 22 row blocks: with max_keep = 1 the chunks are 1 + 4 + 16 + 1 row blocks
BATCH_SIZES = (1345, 64, 65, 129)
BATCH_THRESH = F32(0.2)
BATCH_SAMPLES = ("identical", "disjoint", "chain", "tiny0.01", "cars")


def max_keeps(n):
    return (0, 1, 2, 31, 32, 33, 64, n, n + 5)


def batch_case(n):
    """[5, n, 7]: five unlike samples for one fv2p_nms_batch call.  identical never finds a second survivor (every chunk runs), disjoint and
    chain fill any max_keep from their first rows, the tiny and the car sample stop somewhere in between."""
    return np.stack([identical(n, 0.3)[0], disjoint(n)[0], chain(n)[0], tiny(0.01, n=n, seed=40), car_boxes(41, n, sigma=6.0)])
