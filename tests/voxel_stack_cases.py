"""Cases and the expectation of the stacked voxeliser (points_to_voxel_stack), shared by tests/test_voxel_stack_cpu.py (which holds the
expectation builder against direct per-cloud calls) and tests/test_voxel_stack_gpu.py (which holds the HIP kernels against it)."""
import numpy as np

import oracle


def expect(clouds, voxel_size, coors_range, max_points, max_voxels, ndim=None):
    """The collated batch of dataset.collate_batch over the oracle's per-cloud voxelisation: (voxels [sum M, max_points, ndim] f32,
    coords [sum M, 4] (b, z, y, x) i32, num_points [sum M] i32, voxel_cnt [B] i32).  An empty cloud contributes no row."""
    ndim = clouds[0].shape[1] if ndim is None else ndim
    vs, cs, ks, cnt = [np.zeros((0, max_points, ndim), np.float32)], [np.zeros((0, 4), np.int32)], [np.zeros((0,), np.int32)], []
    for b, pts in enumerate(clouds):
        if pts.shape[0] == 0:
            cnt.append(0)
            continue
        v, c, k = oracle.points_to_voxel(np.ascontiguousarray(pts, dtype=np.float32), voxel_size, coors_range, max_points, max_voxels)
        vs.append(v)
        cs.append(np.concatenate([np.full((c.shape[0], 1), b, np.int32), c.astype(np.int32)], 1))
        ks.append(k.astype(np.int32))
        cnt.append(c.shape[0])
    return np.concatenate(vs), np.concatenate(cs), np.concatenate(ks), np.asarray(cnt, np.int32)


def mean_of(voxels, num_points):
    """MeanVFE in float32, slot by slot in slot order as fv2p_voxel_mean_collate sums (vfe/mean_vfe.py:14-31)."""
    s = np.zeros((voxels.shape[0], voxels.shape[2]), np.float32)
    for p in range(voxels.shape[1]):
        s = (s + voxels[:, p, :]).astype(np.float32)
    return (s / np.maximum(num_points, 1).astype(np.float32)[:, None]).astype(np.float32)


def random_geometry(seed):
    """The geometries of test_voxeliser_random_geometries_match_oracle (tests/test_voxel_gpu.py) - random range, voxel size, feature width 3
    to 6, a fifth of the points on cell faces, points outside the range - as a stack of 2 to 6 clouds.  max_voxels is drawn around the
    clouds' typical distinct-voxel count (a quarter to one and a half times the median of a cheap estimate), so that the break is hit in a
    good share of the samples and missed in the others.  -> (clouds, voxel_size, range, max_points, max_voxels)"""
    rng = np.random.default_rng(1000 + seed)
    lo = rng.uniform(-50, 0, 3).astype(np.float32)
    vs = rng.choice([0.05, 0.1, 0.16, 0.2, 0.4], 3).astype(np.float32)
    cells = rng.integers(3, 60, 3)
    rng_arr = np.concatenate([lo, lo + vs * cells]).astype(np.float32)
    ndim, b = int(rng.integers(3, 7)), int(rng.integers(2, 7))
    clouds, distinct = [], []
    for _ in range(b):
        n = int(rng.integers(1, 6000))
        pts = rng.uniform(-0.1, 1.1, (n, ndim)).astype(np.float32)
        pts[:, :3] = lo + pts[:, :3] * (rng_arr[3:] - lo)
        snap = rng.random(n) < 0.2
        pts[snap, :3] = (lo + np.round((pts[snap, :3] - lo) / vs) * vs).astype(np.float32)
        clouds.append(pts)
        cell = np.floor((pts[:, :3] - lo) / vs).astype(np.int64)
        inside = np.all((cell >= 0) & (cell < cells), axis=1)
        distinct.append(len(np.unique(cell[inside], axis=0)))
    mp = int(rng.integers(1, 9))
    mv = max(1, int(np.median(distinct) * rng.uniform(0.25, 1.5)))
    return clouds, vs, rng_arr, mp, mv
