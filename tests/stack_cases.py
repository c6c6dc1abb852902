"""Cases and plain numpy references for the stacked pointnet2 ops (tests/test_pointnet2_stack_cpu.py, tests/test_pointnet2_stack_gpu.py).

Plain module: no fixtures, no import of `oracle` or of the library.  Everything is generated from a seed.

Two coordinate families:

* ``lattice``: every coordinate is an integer multiple of 1/64 with |x| <= 8.  A difference is then k/64 with |k| <= 1024, a square
  k^2 / 4096 with k^2 <= 2^20 and a three-term sum stays below 2^22 / 4096: every operation of the squared distance is EXACT in float32,
  so float32 in any operand order and float64 give the same number and `d2 == r2` can be planted on purpose (radii 0.5 and 1.25: the
  squares 0.25 and 1.5625 are dyadic).  The box is tighter than "|x| < 64" because a difference of 128 squared needs 26 bits.
* ``generic``: uniform float32 coordinates; a borderline pair is decided by the float32 operation order ((dx*dx + dy*dy) + dz*dz,
  every operation rounded) and by nothing else.

The references restate what the ops MEAN, vectorised per sample, with no loop structure in common with the kernels:
ball query = first `nsample` rows of the query's own sample with d2 < r2 in row order, the remaining slots repeat the first hit, an empty
ball is -1 in slot 0 over the caller's zero fill; voxel query = the same with d2 <= r2 over the occupied voxels of the clipped
neighbourhood in z, y, x scan order, GLOBAL rows; 3-NN = the three smallest by (distance, row), GLOBAL rows, and for a sample with fewer
than three known points the untouched slots keep squared distance +inf and the sample's FIRST global row (see ref_three_nn)."""
import numpy as np

STEP = 1.0 / 64.0
U32 = 2.0 ** -24          # unit roundoff of float32

# ---- layouts: (known points per sample, queries per sample) ------------------------------------------------------------------------
LAYOUTS = {
    "one": ([1500], [300]),
    "one_grid": ([3500], [300]),                                     # >= 3000 known points per sample: three_nn takes its grid search
    "today": ([3000, 1, 2500], [300, 200, 290]),                     # tests/test_pointnet2_gpu.py::test_stack_ops
    "zero_queries_mid": ([500, 700, 400], [260, 0, 130]),
    "zero_queries_end": ([600, 300], [200, 0]),
    "zero_queries_first": ([300, 600], [0, 150]),
    "zero_points_mid": ([400, 0, 300], [100, 50, 120]),              # every ball of sample 1 empty, its 3-NN slots untouched
    "zero_points_first": ([0, 300], [70, 60]),
    "forty_samples": ([30] * 40, [7] * 40),                          # the first 256-query workgroup spans 37 samples
    "queries_1": ([200], [1]),
    "queries_255": ([300, 200], [128, 127]),
    "queries_256": ([300, 200], [128, 128]),
    "queries_257": ([300, 200], [128, 129]),
    "queries_63": ([100, 90, 80], [21, 21, 21]),                     # the 3-NN workgroup serves 64 queries
    "queries_64": ([100, 90, 80], [21, 22, 21]),
    "queries_65": ([100, 90, 80], [22, 22, 21]),
    "points_1023": ([1023, 50], [40, 30]),                           # the kernels stage 1024 points per tile
    "points_1024": ([1024, 50], [40, 30]),
    "points_1025": ([50, 1025], [30, 40]),
    "points_2048": ([2048, 50], [40, 30]),
    "points_2049": ([50, 2049], [30, 40]),
    "few_known": ([1, 2, 500], [30, 30, 30]),                        # fewer than three neighbours
}
# layouts that also run on the generic family
GENERIC_LAYOUTS = ["one", "one_grid", "today", "zero_queries_mid", "zero_points_mid", "forty_samples", "queries_257", "queries_65",
                   "points_1025", "points_2048", "few_known"]
NSAMPLES = [1, 5, 16, 32, 64, 100]
CHANNELS = [1, 3, 16, 67, 128]
RADII = [0.5, 1.25]

REMOTE_A = np.float32([6.0, 6.0, 6.0])       # outside the clouds' box [-3, 3]^3 by more than any radius used
REMOTE_B = np.float32([-6.0, 6.0, -6.0])
REMOTE_C = np.float32([6.0, -6.0, -6.0])


def _coords(rng, n, family, lo=-3.0, hi=3.0):
    if family == "lattice":
        return (rng.integers(int(round(lo * 64)), int(round(hi * 64)) + 1, (n, 3)) * STEP).astype(np.float32)
    return rng.uniform(lo, hi, (n, 3)).astype(np.float32)


def at_radius_offsets(radius):
    """Lattice offsets of length EXACTLY `radius` (a multiple of 1/64): the axis ones, and a 3-4-5 triple when the radius allows it."""
    k = int(round(radius * 64))
    assert k * STEP == radius, "lattice radii are multiples of 1/64"
    offs = [(k, 0, 0), (0, k, 0), (0, 0, -k)]
    if k % 5 == 0:
        offs.append((3 * k // 5, 4 * k // 5, 0))
    return [np.float32(o) * np.float32(STEP) for o in offs]


def cloud_case(layout, family, radius=0.5, seed=0):
    """-> dict(xyz, xyz_cnt, new_xyz, new_cnt, radius, planted).  `planted` maps a tag to stacked query rows:
    'one_hit_last' (the only point inside the ball is the sample's LAST row; one point sits at exactly d2 == r2 and one a lattice step
    outside), 'only_at_radius' (every candidate at exactly d2 == r2: an empty ball under '<'), 'remote' (nothing near), 'tie3' (three
    known points at exactly the same distance and a fourth equidistant one with a higher row)."""
    pts_cnt, qry_cnt = LAYOUTS[layout]
    rng = np.random.default_rng([seed, sorted(LAYOUTS).index(layout), int(family == "lattice"), int(round(radius * 64))])
    lat = family == "lattice"
    r = np.float32(radius)
    pts, qrys, planted = [], [], {"one_hit_last": [], "only_at_radius": [], "remote": [], "tie3": []}
    row = 0
    for n, m in zip(pts_cnt, qry_cnt):
        p, q = _coords(rng, n, family), _coords(rng, m, family)
        small = lambda k: ((rng.integers(-8, 9, (k, 3)) * STEP) if lat else rng.uniform(-0.1, 0.1, (k, 3))).astype(np.float32)
        if 1 <= n <= 2 and m:
            q = (p[0] + small(m)).astype(np.float32)            # everybody's nearest: one row collects every contribution
        elif n >= 10 and m >= 8:
            c0, c1 = m // 2, m // 2 + max(m // 8, 1)
            q[c0:c1] = p[n // 2] + small(c1 - c0)               # a clump of queries sharing their neighbours
            if lat:
                offs = at_radius_offsets(radius)
                q[0] = REMOTE_A
                p[n - 1] = REMOTE_A + np.float32([r - STEP, 0, 0])
                p[0] = REMOTE_A + offs[0]
                p[1] = REMOTE_A - np.float32([r + STEP, 0, 0])
                q[1] = REMOTE_B
                for j, o in enumerate(offs[1:]):
                    p[2 + j] = REMOTE_B + o
                planted["only_at_radius"].append(row + 1)
                s4 = np.float32(4 * STEP)
                q[3] = p[5] + np.float32([s4, 0, 0])
                p[6] = p[5] + np.float32([2 * s4, 0, 0])
                p[7] = p[5] + np.float32([s4, s4, 0])
                p[n - 2] = p[5] + np.float32([s4, -s4, 0])
                planted["tie3"].append(row + 3)
            else:
                q[0] = REMOTE_A
                p[n - 1] = REMOTE_A + np.float32([0.5 * r, 0, 0])
            q[2] = REMOTE_C
            planted["one_hit_last"].append(row)
            planted["remote"].append(row + 2)
        pts.append(p)
        qrys.append(q)
        row += m
    xyz = np.ascontiguousarray(np.concatenate(pts).astype(np.float32).reshape(-1, 3))
    new_xyz = np.ascontiguousarray(np.concatenate(qrys).astype(np.float32).reshape(-1, 3))
    assert np.abs(xyz).max(initial=0) <= 8 and np.abs(new_xyz).max(initial=0) <= 8
    return dict(xyz=xyz, xyz_cnt=np.array(pts_cnt, np.int32), new_xyz=new_xyz, new_cnt=np.array(qry_cnt, np.int32), radius=float(radius),
                planted=planted, family=family, layout=layout)


# the dense layouts get the combinations that need many hits (more than 64, more than nsample = 100)
_DENSE = {("today", "lattice"): (1.25, 100), ("one_grid", "lattice"): (1.25, 64), ("points_2049", "lattice"): (1.25, 32),
          ("today", "generic"): (1.25, 64), ("one_grid", "generic"): (1.25, 100)}


def _covering(layouts, family, k0):
    """(layout, family, radius, nsample): radii and nsample cycled so that every value meets several kinds of layout."""
    return [(lay, family) + _DENSE.get((lay, family), (RADII[(k0 + i) % 2], NSAMPLES[(k0 + i // 2) % 6])) for i, lay in enumerate(layouts)]


BALL_CASES = _covering(sorted(LAYOUTS), "lattice", 0) + _covering(GENERIC_LAYOUTS, "generic", 1)
NN_CASES = [(lay, "lattice") for lay in sorted(LAYOUTS)] + [(lay, "generic") for lay in GENERIC_LAYOUTS]
# grouping and interpolation (forward, atomic gradient, gather gradient): a subset of the above with the channel counts cycled
GROUP_CASES = [BALL_CASES[i] + (CHANNELS[j % 5],) for j, i in enumerate([0, 3, 5, 9, 13, 16, 18, 20, 21, 23, 24, 27, 29, 32])]
INTERP_CASES = [NN_CASES[i] + (CHANNELS[(j + 2) % 5],) for j, i in enumerate([0, 3, 5, 9, 13, 16, 18, 20, 21, 23, 24, 27, 29, 32])]


def case_id(c):
    return "-".join(str(v) for v in c)


# ---- voxel-query scenes ------------------------------------------------------------------------------------------------------------
GRID = (5, 12, 10)                                    # Z, Y, X
VOXEL = np.float32([0.5, 0.5, 1.0])                   # x, y, z size: multiples of 1/64
ORIGIN = np.float32([-2.5, -3.0, -2.5])
OCCUPANCY = [0.9, 0.35, 0.04]                         # per sample of the batch of three
PLANT_VOXEL = (2, 6, 5)                               # z, y, x of the query whose neighbours are planted at d2 == r2 and one step off it
VOXEL_CASES = [("lattice", (1, 2, 2), 0.5, 16), ("lattice", (1, 2, 2), 1.25, 5), ("lattice", (0, 0, 0), 0.5, 1), ("lattice", (1, 2, 20), 1.25, 100),
               ("lattice", (1, 2, 2), 100.0, 64), ("lattice", (7, 2, 2), 100.0, 32), ("lattice", (1, 2, 2), 0.5, 32),
               ("generic", (1, 2, 2), 0.5, 16), ("generic", (0, 0, 0), 1.25, 5), ("generic", (1, 2, 20), 100.0, 100), ("generic", (1, 2, 2), 1.25, 64),
               ("generic", (2, 1, 1), 0.8, 1)]


def voxel_scene(family, radius, seed=0):
    """-> dict(xyz, xyz_cnt, new_xyz, new_cnt, new_coords (M, 4) [b, z, y, x], vol (3, Z, Y, X) global row or -1, planted rows).
    Rows of a sample are in random order (the scan order of the neighbourhood is not the row order); queries sit in every corner, on every
    face and at random voxels.  On the lattice family the planted query of every sample has, in neighbouring voxels, one point at exactly
    d2 == r2 (accepted here), one a lattice step inside and one a step outside (coordinates are what the op reads: they are not kept
    inside their voxel)."""
    Z, Y, X = GRID
    rng = np.random.default_rng([seed, 77, int(family == "lattice"), int(round(radius * 64))])
    lat = family == "lattice"
    vol = -np.ones((3, Z, Y, X), np.int32)
    pts, cnts, qc, qx, planted = [], [], [], [], []
    row0 = qrow = 0
    pz, py, px = PLANT_VOXEL
    for b in range(3):
        occ = rng.random((Z, Y, X)) < OCCUPANCY[b]
        for v in [(pz, py, px + 1), (pz, py, px - 1), (pz, py + 1, px)]:
            occ[v] = True
        z, y, x = np.nonzero(occ)
        perm = rng.permutation(z.size)
        z, y, x = z[perm], y[perm], x[perm]
        inside = (rng.integers(0, 32, (z.size, 3)) * STEP) if lat else rng.uniform(0, 0.5, (z.size, 3))
        p = (ORIGIN + np.stack([x, y, z], 1) * VOXEL + inside * np.float32([1, 1, 2])).astype(np.float32)
        vol[b, z, y, x] = row0 + np.arange(z.size)
        centre = lambda zz, yy, xx: (ORIGIN + (np.float32([xx, yy, zz]) + np.float32(0.5)) * VOXEL).astype(np.float32)
        if lat and radius <= 2:
            r = np.float32(radius)
            c = centre(pz, py, px)
            p[vol[b, pz, py, px + 1] - row0] = c + np.float32([r, 0, 0])
            p[vol[b, pz, py, px - 1] - row0] = c - np.float32([r + STEP, 0, 0])
            p[vol[b, pz, py + 1, px] - row0] = c + np.float32([0, r - STEP, 0])
        corners = [(zz, yy, xx) for zz in (0, Z - 1) for yy in (0, Y - 1) for xx in (0, X - 1)]
        faces = [(0, Y // 2, X // 2), (Z - 1, Y // 2, X // 2), (Z // 2, 0, X // 2), (Z // 2, Y - 1, X // 2), (Z // 2, Y // 2, 0), (Z // 2, Y // 2, X - 1)]
        rand = [tuple(v) for v in np.stack([rng.integers(0, Z, 40 + 15 * b), rng.integers(0, Y, 40 + 15 * b), rng.integers(0, X, 40 + 15 * b)], 1)]
        vox = [PLANT_VOXEL] + corners + faces + rand
        planted.append(qrow)
        q = np.stack([centre(*v) for v in vox])
        if not lat:
            q[1:] += rng.uniform(-0.2, 0.2, (len(vox) - 1, 3)).astype(np.float32)
        qc.append(np.array([(b,) + v for v in vox], np.int32))
        qx.append(q.astype(np.float32))
        pts.append(p)
        cnts.append(z.size)
        row0 += z.size
        qrow += len(vox)
    return dict(xyz=np.ascontiguousarray(np.concatenate(pts)), xyz_cnt=np.array(cnts, np.int32), new_xyz=np.ascontiguousarray(np.concatenate(qx)),
                new_cnt=np.array([len(c) for c in qc], np.int32), new_coords=np.ascontiguousarray(np.concatenate(qc)), vol=vol,
                planted=planted, family=family, radius=float(radius))


# ---- references --------------------------------------------------------------------------------------------------------------------
def d2_f32(a, b):
    """(Na, 3) x (Nb, 3) -> (Na, Nb) float32: (dx*dx + dy*dy) + dz*dz, rounded after every operation."""
    d = (a[:, None, :] - b[None, :, :]).astype(np.float32)
    sq = (d * d).astype(np.float32)
    return ((sq[..., 0] + sq[..., 1]).astype(np.float32) + sq[..., 2]).astype(np.float32)


def d2_f64(a, b):
    d = a[:, None, :].astype(np.float64) - b[None, :, :].astype(np.float64)
    return (d * d).sum(-1)


def r2_of(radius):
    """The threshold the ops compare with: the float32 product of the float32 radius."""
    return np.float32(radius) * np.float32(radius)


def sample_blocks(cnt):
    """-> [(start, stop)] of every sample in a stacked array."""
    stops = np.cumsum(np.asarray(cnt, np.int64))
    return list(zip((stops - cnt).tolist(), stops.tolist()))


def _fill_hits(out, row, hits, nsample):
    hits = hits[:nsample]
    if hits.size == 0:
        out[row, 0] = -1
    else:
        out[row, :] = hits[0]
        out[row, :hits.size] = hits


def ref_ball_query(case, nsample, d2fn):
    """Raw op output (M, nsample) int32, rows LOCAL to the sample; d2fn = d2_f64 (exact on the lattice family) or d2_f32."""
    r2 = r2_of(case["radius"])
    out = np.zeros((case["new_xyz"].shape[0], nsample), np.int32)
    hits_per_query = np.zeros(out.shape[0], np.int64)
    for (p0, p1), (q0, q1) in zip(sample_blocks(case["xyz_cnt"]), sample_blocks(case["new_cnt"])):
        hit = d2fn(case["new_xyz"][q0:q1], case["xyz"][p0:p1]) < r2
        hits_per_query[q0:q1] = hit.sum(1)
        for i in range(q1 - q0):
            _fill_hits(out, q0 + i, np.flatnonzero(hit[i]), nsample)
    return out, hits_per_query


def ambiguous_ball(case):
    """Queries with a candidate whose float64 d2 lies within 4 * 2^-24 * max(d2, r2) of r2."""
    r2 = float(r2_of(case["radius"]))
    amb = np.zeros(case["new_xyz"].shape[0], bool)
    for (p0, p1), (q0, q1) in zip(sample_blocks(case["xyz_cnt"]), sample_blocks(case["new_cnt"])):
        d = d2_f64(case["new_xyz"][q0:q1], case["xyz"][p0:p1])
        amb[q0:q1] = (np.abs(d - r2) <= 4 * U32 * np.maximum(d, r2)).any(1)
    return amb


def _neighbourhood(scene, q, max_range):
    """Occupied voxels of the clipped neighbourhood of query q in z, y, x scan order -> global rows."""
    Z, Y, X = GRID
    b, cz, cy, cx = (int(v) for v in scene["new_coords"][q])
    rz, ry, rx = max_range
    blk = scene["vol"][b, max(cz - rz, 0):min(cz + rz, Z - 1) + 1, max(cy - ry, 0):min(cy + ry, Y - 1) + 1, max(cx - rx, 0):min(cx + rx, X - 1) + 1]
    rows = blk.reshape(-1)
    return rows[rows >= 0]


def ref_voxel_query(scene, max_range, nsample, d2fn):
    """Raw op output (M, nsample) int32, GLOBAL rows; accepts d2 <= r2."""
    r2 = r2_of(scene["radius"])
    m = scene["new_coords"].shape[0]
    out = np.zeros((m, nsample), np.int32)
    hits_per_query = np.zeros(m, np.int64)
    for q in range(m):
        rows = _neighbourhood(scene, q, max_range)
        d = d2fn(scene["new_xyz"][q:q + 1], scene["xyz"][rows])[0]
        hits = rows[d <= r2]
        hits_per_query[q] = hits.size
        _fill_hits(out, q, hits, nsample)
    return out, hits_per_query


def ambiguous_voxel(scene, max_range):
    r2 = float(r2_of(scene["radius"]))
    amb = np.zeros(scene["new_coords"].shape[0], bool)
    for q in range(amb.size):
        d = d2_f64(scene["new_xyz"][q:q + 1], scene["xyz"][_neighbourhood(scene, q, max_range)])[0]
        amb[q] = (np.abs(d - r2) <= 4 * U32 * np.maximum(d, r2)).any()
    return amb


def ref_three_nn(case, d2fn):
    """-> (d2 (N, 3) float32, idx (N, 3) int32 GLOBAL rows into xyz): the three smallest by (distance, row).

    Fewer than three known points in the query's sample (the reference's three_nn_kernel_stack, interpolate_gpu.cu of pointnet2_stack):
    the running best distances start at 1e40 (double) and the best rows at 0; slots no candidate displaced are written out as they
    are, the distance cast to float (+inf) and the row as 0 + the sample's first global row.  So an untouched slot holds (+inf, first row
    of the sample) - for a sample WITHOUT points that is the first row of the next sample, or the total row count behind the last one."""
    n = case["new_xyz"].shape[0]
    d2 = np.full((n, 3), np.inf, np.float32)
    idx = np.zeros((n, 3), np.int32)
    for (p0, p1), (q0, q1) in zip(sample_blocks(case["xyz_cnt"]), sample_blocks(case["new_cnt"])):
        idx[q0:q1] = p0
        k = min(3, p1 - p0)
        if k == 0 or q1 == q0:
            continue
        d = d2fn(case["new_xyz"][q0:q1], case["xyz"][p0:p1])
        order = np.argsort(d, axis=1, kind="stable")[:, :k]          # stable: equal distances stay in row order
        idx[q0:q1, :k] = order + p0
        d2[q0:q1, :k] = np.take_along_axis(d, order, 1).astype(np.float32)
    return d2, idx


def ambiguous_three_nn(case):
    """Queries where another candidate's float64 d2 lies within 4 * 2^-24 * max of the third or of the fourth best distance."""
    amb = np.zeros(case["new_xyz"].shape[0], bool)
    for (p0, p1), (q0, q1) in zip(sample_blocks(case["xyz_cnt"]), sample_blocks(case["new_cnt"])):
        if p1 - p0 < 2 or q1 == q0:
            continue
        s = np.sort(d2_f64(case["new_xyz"][q0:q1], case["xyz"][p0:p1]), 1)[:, :5]
        s = np.concatenate([s, np.full((s.shape[0], 5 - s.shape[1]), np.inf)], 1)
        with np.errstate(invalid="ignore"):
            gap = s[:, 2:5] - s[:, 1:4]                                # second-third, third-fourth, fourth-fifth
            amb[q0:q1] = (np.isfinite(gap) & (gap <= 4 * U32 * s[:, 2:5])).any(1)   # a missing neighbour (inf) is no candidate
    return amb


def global_rows(case, idx_local):
    """Sample-local rows of every query (M, S) -> global rows into xyz."""
    starts = np.array([b[0] for b in sample_blocks(case["xyz_cnt"])], np.int64)
    return idx_local.astype(np.int64) + np.repeat(starts, case["new_cnt"])[:, None]


def ref_group(features, rows):
    """features (N, C), rows (M, S) global -> (M, C, S): pure indexing."""
    return np.ascontiguousarray(features[rows].transpose(0, 2, 1))


def ref_group_grad(grad_out, rows, n):
    """grad_out (M, C, S) -> (sum (n, C) float64, sum of absolute values (n, C), contributions per row (n,))."""
    g = grad_out.astype(np.float64).transpose(0, 2, 1).reshape(-1, grad_out.shape[1])
    want, mag = np.zeros((n, grad_out.shape[1])), np.zeros((n, grad_out.shape[1]))
    np.add.at(want, rows.reshape(-1), g)
    np.add.at(mag, rows.reshape(-1), np.abs(g))
    return want, mag, np.bincount(rows.reshape(-1), minlength=n)


def ref_interp(features, idx, weight):
    """-> (sum_j w_j f_j (N, C) float64, sum_j |w_j f_j|)."""
    t = weight.astype(np.float64)[:, :, None] * features.astype(np.float64)[idx]
    return t.sum(1), np.abs(t).sum(1)


def ref_interp_grad(grad_out, idx, weight, m):
    want, mag = np.zeros((m, grad_out.shape[1])), np.zeros((m, grad_out.shape[1]))
    for j in range(3):
        t = grad_out.astype(np.float64) * weight.astype(np.float64)[:, j:j + 1]
        np.add.at(want, idx[:, j], t)
        np.add.at(mag, idx[:, j], np.abs(t))
    return want, mag, np.bincount(idx.reshape(-1), minlength=m)
